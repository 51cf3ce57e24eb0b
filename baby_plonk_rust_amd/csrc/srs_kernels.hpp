// srs_kernels.hpp -- SRS ingest / export / generation on the GPU.
//   srs_decode96   : 96-byte zkcrypto uncompressed encoding (g1.rs:246-322) -> device Montgomery affine
//   srs_encode96   : the inverse (G1Affine::to_uncompressed)
//   srs_generate   : P_i = s_i * G with s_i = tau^i (Setup::generate_srs, setup.rs:12-31) or
//                    s_i = a + i*d (synthetic benchmark points)
//   srs_decode48 / srs_subgroup_check / srs_encode48 : the 48-byte compressed encoding (g1.rs:221-244, 326-390) and the subgroup
//                    test (g1.rs:401-411), arithmetic in g1_check.hpp
//   srs_scale      : out_i = k_i P_i, one variable-base multiplication per lane (a ceremony contribution, bp_srs_scale)
//   g1_ntt_pass    : one pass of the inverse transform over G1 (bp_srs_lagrange); g1_ntt_table_pass0 / _toeplitz_pass0 / _final_pass0 and
//                    open_all_chat_fill: pass 0 of the three transforms behind bp_kzg_open_all and its scalar layout (kzg_open_all.hpp)
//   g1_ntt_cosets_* : the cell proofs of bp_kzg_open_cosets (kzg_open_cosets.hpp): the l side-by-side table transforms
//                    (g1_ntt_cosets_table_pass0, g1_ntt_batch_pass), the two-products-per-lane multiplication and the halving
//                    additions (g1_ntt_cosets_mul_pass, g1_ntt_cosets_halve_pass), the scalar and value layouts
#pragma once
#include "g1.hpp"
#include "g1_28.hpp"
#include "g1_check.hpp"
#include "g1_mul_split28.hpp"
#include "g1_ntt.hpp"
#include "kzg_open_all.hpp"
#include "kzg_open_cosets.hpp"

namespace bp {

__device__ __forceinline__ bool fp_lt_modulus(const fp_t& a) {
  fp_t t;
  return big_sub(t, a, Fp::modulus()) != 0;
}
// 48 big-endian bytes -> canonical limbs (fp.rs:179-190)
__device__ __forceinline__ fp_t fp_from_be48(const uint8_t* b) {
  fp_t r;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    const uint8_t* p = b + 4 * (11 - i);
    r.l[i] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
  }
  return r;
}
__device__ __forceinline__ void fp_to_be48(uint8_t* b, const fp_t& a) {
#pragma unroll
  for (int i = 0; i < 12; i++) {
    uint8_t* p = b + 4 * (11 - i);
    p[0] = (uint8_t)(a.l[i] >> 24); p[1] = (uint8_t)(a.l[i] >> 16); p[2] = (uint8_t)(a.l[i] >> 8); p[3] = (uint8_t)a.l[i];
  }
}

// status: bit 0 = non-canonical coordinate or bad flag bits, bit 1 = point not on the curve
__global__ void __launch_bounds__(256) srs_decode96(const uint8_t* __restrict__ in, size_t n, g1_affine* __restrict__ out,
                                                     uint32_t* __restrict__ status) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t buf[96];
  const uint32_t* src = reinterpret_cast<const uint32_t*>(in + 96 * i);   // 96*i is 4-byte aligned
#pragma unroll
  for (int j = 0; j < 24; j++) {
    uint32_t w = src[j];
    buf[4 * j] = (uint8_t)w; buf[4 * j + 1] = (uint8_t)(w >> 8); buf[4 * j + 2] = (uint8_t)(w >> 16); buf[4 * j + 3] = (uint8_t)(w >> 24);
  }
  const uint32_t flags = buf[0] >> 5;              // compression | infinity | sort   (g1.rs:275-277)
  buf[0] &= 0x1f;
  fp_t x = fp_from_be48(buf), y = fp_from_be48(buf + 48);
  uint32_t bad = 0;
  if (!fp_lt_modulus(x) || !fp_lt_modulus(y)) bad |= 1;
  if (flags & 0b101) bad |= 1;                     // compressed / sort flag on an uncompressed point
  g1_affine p;
  if (flags & 0b010) {                             // infinity: coordinates must be zero (g1.rs:313-314)
    if (!big_is_zero(x) || !big_is_zero(y)) bad |= 1;
    p.x = Fp::zero();
    p.y = Fp::zero();
  } else {
    Fp::to_mont(p.x, x);
    Fp::to_mont(p.y, y);
    fp_t lhs, rhs, b4;                             // y^2 == x^3 + 4  (g1.rs:101-106)
    Fp::sqr(lhs, p.y);
    Fp::sqr(rhs, p.x);
    Fp::mul(rhs, rhs, p.x);
    b4 = Fp::one();
    Fp::dbl(b4, b4);
    Fp::dbl(b4, b4);
    Fp::add(rhs, rhs, b4);
    if (!big_eq(lhs, rhs)) bad |= 2;
  }
  if (bad) atomicOr(status, bad);
  out[i] = p;
}

__global__ void __launch_bounds__(256) srs_encode96(const g1_affine* __restrict__ in, size_t n, uint8_t* __restrict__ out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g1_affine p = in[i];
  uint8_t buf[96];
  if (g1_affine_is_identity(p)) {
#pragma unroll
    for (int j = 0; j < 96; j++) buf[j] = 0;
    buf[0] = 0x40;
  } else {
    fp_t x, y;
    Fp::from_mont(x, p.x);
    Fp::from_mont(y, p.y);
    fp_to_be48(buf, x);
    fp_to_be48(buf + 48, y);
  }
  uint32_t* dst = reinterpret_cast<uint32_t*>(out + 96 * i);
#pragma unroll
  for (int j = 0; j < 24; j++)
    dst[j] = (uint32_t)buf[4 * j] | ((uint32_t)buf[4 * j + 1] << 8) | ((uint32_t)buf[4 * j + 2] << 16) | ((uint32_t)buf[4 * j + 3] << 24);
}

// ---- compressed points (round 7) ------------------------------------------------------------------------------------------------
// One lane per point.  status: a 64-bit word the host sets to ~0; a failing lane does ONE atomicMin of (index << 2) | reason
// (g1_check.hpp: 1 encoding, 2 not on the curve, 3 not in the subgroup), so one 8-byte read gives the lowest failing index and its
// reason -- for the same index a decoding failure (1, 2) wins over the subgroup test, which sees the identity it leaves there.
__device__ __forceinline__ void srs_report(unsigned long long* status, size_t i, uint32_t reason) {
  atomicMin(status, ((unsigned long long)i << 2) | reason);
}
// G1Affine::from_compressed_unchecked (g1.rs:337-390): 48-byte records -> the device Montgomery affine form srs_decode96 writes
__global__ void __launch_bounds__(256) srs_decode48(const uint8_t* __restrict__ in, size_t n, g1_affine* __restrict__ out,
                                                     unsigned long long* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4* src = reinterpret_cast<const uint4*>(in + 48 * i);          // 48 i is 16-byte aligned (in: a hipMalloc workspace)
  uint32_t w[12];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const uint4 v = src[j];
    w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
  }
  g1_affine p;
  const uint32_t bad = g1_decode48(p, w);
  if (bad) srs_report(status, i, bad);
  out[i] = p;
}
// is_torsion_free (g1.rs:401-411) of resident points (the identity (0, 0) passes)
__global__ void __launch_bounds__(256) srs_subgroup_check(const g1_affine* __restrict__ pts, size_t n, unsigned long long* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (!g1_is_torsion_free(pts[i])) srs_report(status, i, G1_NOT_IN_SUBGROUP);
}
// G1Affine::to_compressed (g1.rs:221-244): the compressed twin of srs_encode96
__global__ void __launch_bounds__(256) srs_encode48(const g1_affine* __restrict__ in, size_t n, uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[12];
  g1_encode48(w, in[i]);
  uint4* dst = reinterpret_cast<uint4*>(out + 48 * i);
#pragma unroll
  for (int j = 0; j < 3; j++) dst[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
}

// G1Projective memory images (x | y | z Montgomery limbs, g1.rs:442-446) -> affine, the device side of
// bp_srs_load_projective144.  One lane normalises `group` points with one shared inversion (Montgomery's trick,
// G1Projective::batch_normalize g1.rs:806-839); z = 0 (the identity) becomes (0, 0).  The inversion (a 381-bit power, ~570
// multiplications) is most of what the kernel costs: one per 8 points made 131 072 of them at 2^20 points, 1.77 ms; one per 16: 1.1 ms.  A lane's points are
// `lanes` apart (lane, lane + lanes, ...: neighbouring lanes read neighbouring points) and the running products z'_0 ... z'_j wait in
// the x field of the output slot j, so the group can be as long as the launch wants.
__global__ void __launch_bounds__(256) srs_from_projective(const g1_proj* __restrict__ in, size_t n, uint32_t group, g1_affine* __restrict__ out) {
  const size_t lanes = (n + group - 1) / group;
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= lanes) return;
  fp_t run = Fp::one();
  uint32_t cnt = 0;
  for (size_t i = lane; i < n; i += lanes, cnt++) {
    fp_t z = in[i].z;
    if (big_is_zero(z)) z = Fp::one();                  // z' = z, or 1 where z = 0
    if (cnt == 0) run = z; else Fp::mul(run, run, z);
    out[i].x = run;
  }
  fp_t inv;
  fp_invert_via28(inv, run);
  for (uint32_t j = cnt; j-- > 0;) {
    const size_t i = lane + (size_t)j * lanes;
    const g1_proj p = in[i];
    const bool inf = big_is_zero(p.z);
    fp_t z = p.z, zinv;
    if (inf) z = Fp::one();
    if (j) {
      const fp_t before = out[i - lanes].x;
      Fp::mul(zinv, inv, before);
    } else {
      zinv = inv;
    }
    Fp::mul(inv, inv, z);
    g1_affine r;
    Fp::mul(r.x, p.x, zinv);
    Fp::mul(r.y, p.y, zinv);
    if (inf) { r.x = Fp::zero(); r.y = Fp::zero(); }
    out[i] = r;
  }
}

// ---- a different scalar for every point (bp_srs_scale) ---------------------------------------------------------------------------
// out[i] = k_i * pts[i] as a G1Projective image for srs_from_projective: one lane per point, the 128-step joint double-and-add of
// g1_mul_split28 (the body and the launch bounds of verify_seg_mul).  k_i: Montgomery, any value < q (0 gives the identity);
// pts[i]: a point of the prime-order subgroup -- the host runs srs_subgroup_check first -- or the identity (0, 0), which stays the
// identity (0 : 1 : 0), z = 0.
__global__ void __launch_bounds__(64) srs_scale(const g1_affine* __restrict__ pts, const fr_t* __restrict__ scalars, size_t n,
                                                 g1_proj* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fr_t k = scalars[i];
  Fr::from_mont(k, k);
  out[i] = g1_proj_from_28(g1_mul_split28(pts[i], k));
}

// ---- fixed-base generation (round 4) --------------------------------------------------------------------------------------------
// P = s G as 32 mixed additions from a table of the generator's multiples,  gen_table[j * 255 + (d - 1)] = d 2^(8 j) G  (j < 32, d = 1 .. 255;
// 28-bit affine slots, 1 MiB, built once per context by srs_gen_table), instead of 255 doublings + ~128 additions on saturated limbs per point;
// a lane makes SRS_GEN_GROUP consecutive points and normalises them with ONE inversion (Montgomery's trick, on the same 28-bit limbs).
// Same points as srs_generate (the unique affine representatives), 82 -> see profiles/r04_table_build_ab.txt.
constexpr uint32_t GEN_WINDOWS = 32, GEN_DIGITS = 255, SRS_GEN_GROUP = 8;
__device__ __forceinline__ void store_affine28_slot(g1_affine28* __restrict__ dst, const F28n& x, const F28n& y) {
  uint32_t w[28];
#pragma unroll
  for (int j = 0; j < N28; j++) { w[j] = x.l[j]; w[N28 + j] = y.l[j]; }
  uint4* q = reinterpret_cast<uint4*>(dst);
#pragma unroll
  for (int j = 0; j < 7; j++) q[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
}
__device__ __forceinline__ g1_affine28 load_affine28_slot(const g1_affine28* __restrict__ p) {
  g1_affine28 r;
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint32_t w[28];
#pragma unroll
  for (int j = 0; j < 7; j++) { const uint4 v = q[j]; w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w; }
#pragma unroll
  for (int j = 0; j < N28; j++) { r.x.l[j] = w[j]; r.y.l[j] = w[N28 + j]; }
  return r;
}
__global__ void __launch_bounds__(256) srs_gen_table(g1_affine28* __restrict__ table) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= GEN_WINDOWS * GEN_DIGITS) return;
  const uint32_t j = t / GEN_DIGITS, d = t % GEN_DIGITS + 1;
  fr_t s = Fr::zero();
  s.l[j >> 2] = d << (8 * (j & 3));                            // the integer d 2^(8 j)
  g1_proj r;
  g1_mul_scalar(r, g1_from_affine(g1_affine_generator()), s);
  const g1_affine28 a = g1_affine_to_28(g1_to_affine(r));
  store_affine28_slot(&table[t], a.x, a.y);
}
// mode 0: s_i = a^i (a = tau, Montgomery);  mode 1: s_i = a + i*d (Montgomery).  out[j] = s_{first + j} G, j < n.
__global__ void __launch_bounds__(256, 2) srs_generate_fb(fr_t a, fr_t d, int mode, size_t first, size_t n, const g1_affine28* __restrict__ gen_table,
                                                          g1_affine* __restrict__ out) {
  const size_t base = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * SRS_GEN_GROUP;
  if (base >= n) return;
  const uint32_t cnt = n - base < SRS_GEN_GROUP ? (uint32_t)(n - base) : SRS_GEN_GROUP;
  g1_proj28 pts[SRS_GEN_GROUP];
  M28 prefix[SRS_GEN_GROUP];
  M28 one;
#pragma unroll
  for (int j = 0; j < N28; j++) one.l[j] = One28::limb(j);
  for (uint32_t k = 0; k < cnt; k++) {
    const size_t i = first + base + k;
    fr_t s;
    if (mode == 0) {
      uint32_t e[2] = {(uint32_t)i, (uint32_t)(i >> 32)};
      Fr::pow(s, a, e, 2);
    } else {
      fr_t idx = Fr::zero(), t;
      idx.l[0] = (uint32_t)i;
      idx.l[1] = (uint32_t)(i >> 32);
      Fr::to_mont(idx, idx);
      Fr::mul(t, idx, d);
      Fr::add(s, a, t);
    }
    Fr::from_mont(s, s);
    g1_proj28 acc = g1_identity28();
    for (uint32_t j = 0; j < GEN_WINDOWS; j++) {
      const uint32_t dg = (s.l[j >> 2] >> (8 * (j & 3))) & 255u;
      if (dg) {
        const g1_affine28 q = load_affine28_slot(&gen_table[j * GEN_DIGITS + dg - 1]);
        g1_add_mixed28(acc, q.x, widen28<PtY28>(q.y));
      }
    }
    pts[k] = acc;
    uint32_t zz = 0;
#pragma unroll
    for (int j = 0; j < N28; j++) zz |= acc.z.l[j];              // s = 0: the accumulator is still (0 : 1 : 0) as written
    prefix[k] = zz ? mul28(k ? prefix[k - 1] : one, acc.z) : (k ? prefix[k - 1] : one);
  }
  M28 inv = fp28_invert(prefix[cnt - 1]);
  for (uint32_t k = cnt; k-- > 0;) {
    uint32_t zz = 0;
#pragma unroll
    for (int j = 0; j < N28; j++) zz |= pts[k].z.l[j];
    g1_affine r;
    if (zz) {
      const M28 zinv = mul28(inv, k ? prefix[k - 1] : one);
      inv = mul28(inv, pts[k].z);
      r.x = fp_from_28(mul28(pts[k].x, zinv));
      r.y = fp_from_28(mul28(pts[k].y, zinv));
    } else {
      r.x = Fp::zero();
      r.y = Fp::zero();
    }
    out[base + k] = r;
  }
}

// ---- Lagrange-basis SRS: one pass of the inverse transform over G1 (g1_ntt.hpp) ---------------------------------------------------
// One lane per butterfly, 2^(log_n - 1) lanes; pass 0 (FIRST) reads the affine SRS, every other pass the projective buffer the pass
// before wrote.  Four waves per workgroup, one per SIMD: the lane keeps a point, the accumulator and the temporaries of the complete
// addition in registers through the 255 steps of its scalar multiplication.  n_inv travels as a kernel argument: the scalar of pass 0
// is the same for the whole grid, and so is the twiddle of a wave in every pass with at least 64 groups (g1_ntt_step's lane order).
template <bool FIRST>
__global__ void __launch_bounds__(256) g1_ntt_pass(uint32_t log_n, uint32_t s, const g1_affine* __restrict__ in, const g1_proj* __restrict__ src,
                                                   g1_proj* __restrict__ dst, const fr_t* __restrict__ tw, fr_t n_inv) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= ((uint64_t)1 << (log_n - 1))) return;
  g1_ntt_pass_at<FIRST>(log_n, s, b, in, src, dst, tw, n_inv);
}

// ---- all n proofs of a polynomial on its domain (kzg_open_all.hpp): pass 0 of its three transforms --------------------------------
// One lane per butterfly, as above; every later pass of the three is g1_ntt_pass<false>.  Bounds: the table pass reads srs[k] only for
// k <= n - 2 (open_all_shat), the Toeplitz pass table[j] and sc[j] for j < 2n, the final pass h[j] for j < n; each writes slots < len.
__global__ void __launch_bounds__(256) g1_ntt_table_pass0(uint32_t log_n, const g1_affine* __restrict__ srs, g1_proj* __restrict__ dst) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= ((uint64_t)1 << log_n)) return;                           // len / 2 = n butterflies
  open_all_table_pass0_at(log_n, b, srs, dst);
}
// the scalar differs from lane to lane, so the branch on its bits in g1_ntt_mul diverges inside a wave: every step then costs the
// doubling and the addition (DESIGN.md 4.8 has the pass times)
__global__ void __launch_bounds__(256) g1_ntt_toeplitz_pass0(uint32_t log_len, const g1_affine* __restrict__ table, const fr_t* __restrict__ sc,
                                                               g1_proj* __restrict__ dst) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= ((uint64_t)1 << (log_len - 1))) return;
  open_all_toeplitz_pass0_at(log_len, b, table, sc, dst);
}
#ifdef BP_EXPERIMENT
// The alternative multiplication of the Toeplitz pass, experiment build only (BP_OPEN_ALL_MUL=split28; tools/kzg_open_all_timing.py
// times it beside the default): g1_mul_split28, the 128-step joint double-and-add of srs_scale on 28-bit limbs, with no branch on a
// scalar bit.  Valid here because the table's entries are DFT images of subgroup points, hence subgroup points.  Device only, so
// the host loop of kzg_open_all.hpp cannot run it; DESIGN.md 4.8 has both pass times and why the default is g1_ntt_mul.
__global__ void __launch_bounds__(256) g1_ntt_toeplitz_pass0_split28(uint32_t log_len, const g1_affine* __restrict__ table, const fr_t* __restrict__ sc,
                                                                       g1_proj* __restrict__ dst) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= ((uint64_t)1 << (log_len - 1))) return;
  const G1NttStep st = g1_ntt_step(log_len, 0, b);
  const uint64_t j0 = g1_ntt_bitrev(st.i0, log_len), j1 = g1_ntt_bitrev(st.i1, log_len);
  fr_t k;
  Fr::from_mont(k, sc[j1]);
  g1_proj v = g1_proj_from_28(g1_mul_split28(table[j1], k));
  Fr::from_mont(k, sc[j0]);
  g1_proj u = g1_proj_from_28(g1_mul_split28(table[j0], k));
  g1_ntt_butterfly(u, v);
  dst[st.i0] = u;
  dst[st.i1] = v;
}
#endif
__global__ void __launch_bounds__(256) g1_ntt_final_pass0(uint32_t log_n, const g1_proj* __restrict__ h, g1_proj* __restrict__ dst) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= ((uint64_t)1 << (log_n - 1))) return;
  open_all_final_pass0_at(log_n, b, h, dst);
}
// out[t] = scale * c^_t, t < 2n (Montgomery): the coefficients f[0 .. n_values) (n_values <= n, the rest zero) laid out for the
// convolution, with N^-1 of the inverse G1 transform already on them
__global__ void __launch_bounds__(256) open_all_chat_fill(uint32_t log_n, const fr_t* __restrict__ f, size_t n_values, fr_t scale, fr_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ((uint64_t)2 << log_n)) return;
  const uint64_t k = open_all_chat(log_n, t);
  fr_t v = Fr::zero();
  if (k != OPEN_ALL_NONE && k < n_values) Fr::mul(v, f[k], scale);
  out[t] = v;
}

// ---- the n / l cell proofs of a polynomial (kzg_open_cosets.hpp) ---------------------------------------------------------------------
// One lane per butterfly or per output point.  Bounds: the table pass reads srs[k] only for k <= n - l - 1 (open_cosets_shat) and
// writes the 2n slots of the l transforms; the batch pass reads and writes inside its own sub-transform; the multiplication reads
// table and sc below 2n and writes dst below n; the halving pass touches buf below 2 half.
__global__ void __launch_bounds__(256) g1_ntt_cosets_table_pass0(uint32_t log_n, uint32_t log_l, const g1_affine* __restrict__ srs,
                                                                   g1_proj* __restrict__ dst) {
  const uint64_t B = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (B >= ((uint64_t)1 << log_n)) return;                           // l transforms of R / 2 = r butterflies
  open_cosets_table_pass0_at(log_n, log_l, B, srs, dst);
}
// pass s >= 1 of 2^log_count transforms of 2^log_len points side by side: the sub-transform is the high bits of the butterfly id
__global__ void __launch_bounds__(256) g1_ntt_batch_pass(uint32_t log_len, uint32_t log_count, uint32_t s, const g1_proj* __restrict__ src,
                                                           g1_proj* __restrict__ dst, const fr_t* __restrict__ tw) {
  const uint64_t B = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (B >= ((uint64_t)1 << (log_len - 1 + log_count))) return;
  open_cosets_batch_pass_at(log_len, s, B, src, dst, tw);
}
// two scalar multiplications per lane, each with a scalar of its own (the divergence of g1_ntt_toeplitz_pass0), and one addition
__global__ void __launch_bounds__(256) g1_ntt_cosets_mul_pass(uint32_t log_n, uint32_t log_l, const g1_affine* __restrict__ table,
                                                                const fr_t* __restrict__ sc, g1_proj* __restrict__ dst) {
  const uint64_t B = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (B >= ((uint64_t)1 << log_n)) return;
  open_cosets_mul_at(log_n, log_l, B, table, sc, dst);
}
__global__ void __launch_bounds__(256) g1_ntt_cosets_halve_pass(uint64_t half, g1_proj* buf) {
  const uint64_t B = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (B >= half) return;
  open_cosets_halve_at(half, B, buf);
}
// out[j R + t] = scale * c^(j)_t (Montgomery): the l columns of the batched Fr transform, from f[0 .. n_values), the rest zero
__global__ void __launch_bounds__(256) open_cosets_chat_fill(uint32_t log_n, uint32_t log_l, const fr_t* __restrict__ f, size_t n_values, fr_t scale,
                                                               fr_t* __restrict__ out) {
  const uint64_t at = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (at >= ((uint64_t)2 << log_n)) return;
  const uint32_t log_R = log_n - log_l + 1;
  const uint64_t k = open_cosets_chat(log_n, log_l, at >> log_R, at & (((uint64_t)1 << log_R) - 1));
  fr_t v = Fr::zero();
  if (k != OPEN_ALL_NONE && k < n_values) Fr::mul(v, f[k], scale);
  out[at] = v;
}
// out[k l + j] = in[k + r j]: the n values f(omega^i) in cell order
__global__ void __launch_bounds__(256) open_cosets_cell_order(uint32_t log_n, uint32_t log_l, const fr_t* __restrict__ in, fr_t* __restrict__ out) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ((uint64_t)1 << log_n)) return;
  out[c] = in[open_cosets_value_source(log_n, log_l, c)];
}

}  // namespace bp

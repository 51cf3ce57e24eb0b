// host_codec.hpp -- the host code that turns field elements and points into the bytes the C ABI returns, and back: the ONE
// definition of every wire format and of the small Fr helpers the translation units share.  Host-only inline functions over
// g1_check.hpp; no HIP call and no bp_ctx, so tests/test_host_codec.py compiles this header alone and checks it on the CPU against
// the crate's fixtures.  (The kernels of srs_kernels.hpp keep their own device copies of the 96-byte forms.)
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/bp_msm_ntt.h"
#include "g1_check.hpp"

namespace bp {

// ---- Fp: 48 big-endian bytes <-> canonical limbs (the byte order of Fp::to_bytes / from_bytes, fp.rs:211-227 / 179-207)
inline void fp_to_be48_host(uint8_t* b, const fp_t& a) {
  for (int i = 0; i < 12; i++) {
    const uint32_t w = __builtin_bswap32(a.l[i]);
    memcpy(b + 4 * (11 - i), &w, 4);
  }
}
inline fp_t fp_from_be48_host(const uint8_t* b) {
  fp_t r;
  for (int i = 0; i < 12; i++) {
    uint32_t w;
    memcpy(&w, b + 4 * (11 - i), 4);
    r.l[i] = __builtin_bswap32(w);
  }
  return r;
}

// ---- G1, 96 bytes
// G1Affine::from(p).to_uncompressed()  (g1.rs:49-63, 246-260)
inline void host_encode96(uint8_t out96[96], const g1_proj& p) {
  memset(out96, 0, 96);
  if (g1_is_identity(p)) {
    out96[0] = 0x40;
    return;
  }
  const g1_affine a = g1_to_affine(p);
  fp_t x, y;
  Fp::from_mont(x, a.x);
  Fp::from_mont(y, a.y);
  fp_to_be48_host(out96, x);
  fp_to_be48_host(out96 + 48, y);
}
// G1Affine::from_uncompressed_unchecked (g1.rs:273-322): canonical coordinates and the flag rules, NO curve check
inline bool host_decode96(g1_proj& out, const uint8_t in96[96]) {
  uint8_t buf[96];
  memcpy(buf, in96, 96);
  const uint32_t flags = buf[0] >> 5;
  buf[0] &= 0x1f;
  fp_t x = fp_from_be48_host(buf), y = fp_from_be48_host(buf + 48), t;
  if (!big_sub(t, x, Fp::modulus()) || !big_sub(t, y, Fp::modulus())) return false;
  if (flags & 0b101) return false;
  if (flags & 0b010) {
    if (!big_is_zero(x) || !big_is_zero(y)) return false;
    out = g1_identity();
    return true;
  }
  Fp::to_mont(out.x, x);
  Fp::to_mont(out.y, y);
  out.z = Fp::one();
  return true;
}
// The equation of G1Affine::is_on_curve (g1.rs:414-417), y^2 = x^3 + 4, and nothing else: the reference's `| self.infinity` is a flag
// of the record, which the caller has (host_decode96 gives z = 0 for it).  The pair (0, 0) that stands for the identity in device
// buffers is NOT on the curve: a record of zero coordinates without the infinity flag is refused here, as the reference refuses it.
inline bool g1_affine_on_curve(const g1_affine& p) {
  fp_t lhs, rhs, b4 = Fp::one();
  Fp::sqr(lhs, p.y);
  Fp::sqr(rhs, p.x);
  Fp::mul(rhs, rhs, p.x);
  Fp::dbl(b4, b4);
  Fp::dbl(b4, b4);
  Fp::add(rhs, rhs, b4);
  return big_eq(lhs, rhs);
}

// ---- G1, 48 bytes.  The sign bit is g1_encode48's (g1_check.hpp), the rule the device encoder uses: y >= (p + 1) / 2.  The
// reference states it as y > -y (fp.rs:273-298); for y != 0 that is y > p - y, i.e. 2 y > p, i.e. y >= (p + 1) / 2 as p is odd, and
// for y = 0 both are false (-0 = 0): one rule.
// G1Affine::from(p).to_compressed()  (g1.rs:49-63, 221-244)
inline void host_compress48(uint8_t out48[48], const g1_proj& p) {
  uint32_t w[12];
  g1_encode48(w, g1_to_affine(p));
  memcpy(out48, w, 48);
}
// k affine forms from ONE field inversion (Montgomery's trick, as G1Projective::batch_normalize does, g1.rs:806-839); the
// identity (z = 0) is skipped and comes out as (0, 0).  out[j].x holds the running product on the way up: no scratch, any k.
inline void host_batch_to_affine(g1_affine* out, const g1_proj* in, int k) {
  fp_t acc = Fp::one(), inv;
  for (int j = 0; j < k; j++) {
    out[j].x = acc;
    if (!g1_is_identity(in[j])) Fp::mul(acc, acc, in[j].z);
  }
  fp_invert(inv, acc);
  for (int j = k; j-- > 0;) {
    if (g1_is_identity(in[j])) {
      out[j].x = out[j].y = Fp::zero();
      continue;
    }
    fp_t zinv;
    Fp::mul(zinv, inv, out[j].x);
    Fp::mul(inv, inv, in[j].z);
    Fp::mul(out[j].x, in[j].x, zinv);
    Fp::mul(out[j].y, in[j].y, zinv);
  }
}
// k compressed records, in blocks of HOST_COMPRESS_BLOCK points: one inversion per block (~26 us on the host, where a Fermat
// inversion is ~570 field products), so one per call for the batches of 3, 1, 3 and 2 a proof compresses
constexpr int HOST_COMPRESS_BLOCK = 16;
inline void host_compress48_many(uint8_t* out, const g1_proj* p, int k) {
  g1_affine a[HOST_COMPRESS_BLOCK];
  for (int base = 0; base < k; base += HOST_COMPRESS_BLOCK) {
    const int m = k - base < HOST_COMPRESS_BLOCK ? k - base : HOST_COMPRESS_BLOCK;
    host_batch_to_affine(a, p + base, m);
    for (int j = 0; j < m; j++) {
      uint32_t w[12];
      g1_encode48(w, a[j]);
      memcpy(out + 48 * (size_t)(base + j), w, 48);
    }
  }
}

// ---- Fr: 32 bytes in either scalar format of the C ABI <-> Montgomery limbs
// BP_FR_BYTES_LE: is the little-endian value below q?  (the test of Scalar::from_bytes, scalar.rs:264-288)
inline bool fr_is_canonical(const uint8_t* b32) {
  fr_t v, t;
  memcpy(&v, b32, 32);
  return big_sub(t, v, Fr::modulus()) != 0;
}
// Scalar::from_bytes (scalar.rs:264-288) for BP_FR_BYTES_LE: false for a value >= q; BP_FR_MONT passes the 32 bytes through
inline bool fr_from_bytes(fr_t& out, const uint8_t* b32, int fmt) {
  if (fmt != BP_FR_MONT && !fr_is_canonical(b32)) return false;
  memcpy(&out, b32, 32);
  if (fmt != BP_FR_MONT) Fr::to_mont(out, out);
  return true;
}
// Scalar::to_bytes (scalar.rs:292-304) for BP_FR_BYTES_LE; BP_FR_MONT copies the limbs
inline void fr_to_bytes(uint8_t* b32, const fr_t& v, int fmt) {
  fr_t t = v;
  if (fmt == BP_FR_BYTES_LE) Fr::from_mont(t, v);
  memcpy(b32, &t, 32);
}
// impl From<u64> for Scalar (scalar.rs:48-52)
inline fr_t fr_from_u64(uint64_t v) {
  fr_t c = Fr::zero(), r;
  c.l[0] = (uint32_t)v;
  c.l[1] = (uint32_t)(v >> 32);
  Fr::to_mont(r, c);
  return r;
}
// Scalar::pow (scalar.rs:381-392) with by = [e, 0, 0, 0], on the host (the kernels have a __device__ function of this name, poly_kernels.hpp)
inline fr_t fr_pow_u64(const fr_t& a, uint64_t e) {
  const uint32_t e32[2] = {(uint32_t)e, (uint32_t)(e >> 32)};
  fr_t r;
  Fr::pow(r, a, e32, 2);
  return r;
}
// root_of_unity (utils.rs:39-43): ROOT_OF_UNITY.pow([2^32 / group_order, 0, 0, 0]) -- integer division, as written; false for
// order 0, where the reference's division panics (`out` is left alone)
inline bool host_root_of_unity(fr_t& out, uint64_t group_order) {
  if (group_order == 0) return false;
  out = fr_pow_u64(fr_root_of_unity(false), ((uint64_t)1 << 32) / group_order);
  return true;
}

}  // namespace bp

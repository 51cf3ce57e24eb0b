// verify_kernels.hpp -- batch verification (Verifier::verify, src/verifier.rs:80-209) up to the two pairings, one proof per lane.
//   plonk_challenges   : the fixed-schedule Fiat-Shamir transcript (compute_challengs, verifier.rs:193-209) as __host__ __device__
//                        code: bp_plonk_challenges on the host and verify_transcript on the device run the same lines
//   verify_transcript  : proof bytes -> the six challenges (Montgomery)
//   verify_scalars     : the coefficient of every base of verifier.rs:86-191 times the proof's weight, column-major
//   verify_shared_sum  : the nine scalars of the bases all proofs share (eight vk points and G), summed over the batch
//   verify_gather      : the 9 m compressed points out of the 624-byte records into column-major order
//
// Why the sponge position is a compile-time constant.  merlin's challenge_bytes ends in STROBE's PRF, whose C flag FORCES a
// permutation when the operation begins (strobe.rs begin_op: `if force_f && pos != 0 { run_f() }`), so every draw reads bytes 0..31
// of a fresh block and leaves (pos, pos_begin) = (32, 0) -- whether it is the first draw of a challenge or the fourteenth, accepted
// or rejected.  The rejection loop of transcript.rs:70-82 therefore changes HOW OFTEN the state is permuted, never WHERE the next
// byte goes: the whole schedule is a type-level cursor Cur<POS, BEGIN>, every byte is XORed into a lane and a shift that the
// compiler sees as constants, and the 25 lanes stay in registers (no LDS image of the state, no masked XORs, no scratch).
#pragma once
#include <type_traits>

#include "../../include/bp_msm_ntt.h"
#include "fields.hpp"

namespace bp {

constexpr int VERIFY_RECORD_BYTES = 624, VERIFY_RECORD_WORDS = 156;     // 9 x 48 + 6 x 32 (bp_prove's encoding)
constexpr int VERIFY_POINTS = 9, VERIFY_EVALS = 6, VERIFY_SHARED = 9;    // proof points, evaluations, shared bases (8 vk + G)

// ---------------------------------------------------------------------------------------------- Keccak-f[1600] in 25 registers
BP_HD uint64_t keccak_rol(uint64_t v, int n) { return n ? (v << n) | (v >> (64 - n)) : v; }
BP_HD constexpr uint64_t keccak_rc(int i) {
  constexpr uint64_t RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull,
                               0x000000000000808Bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
                               0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
                               0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull,
                               0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800Aull, 0x800000008000000Aull,
                               0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
  return RC[i];
}
// one round; every index is a constant, so a[] never leaves the register file
BP_HD void keccak_round(uint64_t (&a)[25], uint64_t rc) {
  constexpr int ROT[5][5] = {{0, 36, 3, 41, 18}, {1, 44, 10, 45, 2}, {62, 6, 43, 15, 61}, {28, 55, 25, 21, 56}, {27, 20, 39, 8, 14}};
  uint64_t c[5], d[5], b[25];
#pragma unroll
  for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
  for (int x = 0; x < 5; x++) d[x] = c[(x + 4) % 5] ^ keccak_rol(c[(x + 1) % 5], 1);
#pragma unroll
  for (int x = 0; x < 5; x++)
#pragma unroll
    for (int y = 0; y < 5; y++) b[y + 5 * ((2 * x + 3 * y) % 5)] = keccak_rol(a[x + 5 * y] ^ d[x], ROT[x][y]);
#pragma unroll
  for (int x = 0; x < 5; x++)
#pragma unroll
    for (int y = 0; y < 5; y++) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
  a[0] ^= rc;
}
// The 24 rounds as a loop of two unrolled rounds: the transcript permutes at ~30 places of straight-line code, and 24 unrolled
// rounds at each of them would be a megabyte of instructions; the round constant is the only thing the loop index selects.
BP_HD void keccak_f1600_regs(uint64_t (&a)[25]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int r = 0; r < 24; r += 2) {
    uint64_t rc0 = 0, rc1 = 0;
#pragma unroll
    for (int k = 0; k < 12; k++) {                 // select, not a table in memory
      rc0 = r == 2 * k ? keccak_rc(2 * k) : rc0;
      rc1 = r == 2 * k ? keccak_rc(2 * k + 1) : rc1;
    }
    keccak_round(a, rc0);
    keccak_round(a, rc1);
  }
}

// ---------------------------------------------------------------------------------------------- STROBE-128 with a type-level cursor
constexpr int STROBE_R = 166;
constexpr uint8_t STROBE_I = 1, STROBE_A = 2, STROBE_C = 4, STROBE_M = 16;
template <int POS, int BEGIN>
struct Cur {
  static constexpr int pos = POS, begin = BEGIN;
};
template <int POS>
BP_HD void strobe_xor(uint64_t (&a)[25], uint8_t v) {
  a[POS >> 3] ^= (uint64_t)v << (8 * (POS & 7));
}
template <int POS, int BEGIN>
BP_HD Cur<0, 0> strobe_run_f(uint64_t (&a)[25], Cur<POS, BEGIN>) {
  strobe_xor<POS>(a, (uint8_t)BEGIN);
  strobe_xor<POS + 1>(a, 0x04);
  strobe_xor<STROBE_R + 1>(a, 0x80);
  keccak_f1600_regs(a);
  return {};
}
template <int POS, int BEGIN>
BP_HD auto strobe_absorb1(uint64_t (&a)[25], Cur<POS, BEGIN> c, uint8_t v) {
  strobe_xor<POS>(a, v);
  if constexpr (POS + 1 == STROBE_R) return strobe_run_f(a, Cur<POS + 1, BEGIN>{});
  else return Cur<POS + 1, BEGIN>{};
}
// n bytes byte_at(integral_constant<int, i>), i < N
template <int N, int I = 0, int POS, int BEGIN, class F>
BP_HD auto strobe_absorb(uint64_t (&a)[25], Cur<POS, BEGIN> c, const F& byte_at) {
  if constexpr (I == N) return c;
  else return strobe_absorb<N, I + 1>(a, strobe_absorb1(a, c, byte_at(std::integral_constant<int, I>{})), byte_at);
}
template <uint8_t FLAGS, int POS, int BEGIN>
BP_HD auto strobe_begin_op(uint64_t (&a)[25], Cur<POS, BEGIN> c) {
  auto c1 = strobe_absorb1(a, Cur<POS, POS + 1>{}, (uint8_t)BEGIN);
  auto c2 = strobe_absorb1(a, c1, FLAGS);
  if constexpr ((FLAGS & STROBE_C) != 0 && decltype(c2)::pos != 0) return strobe_run_f(a, c2);
  else return c2;
}
// meta-AD(label) || meta-AD(len_le32, more): the head of append_message and of challenge_bytes; L = sizeof(label) with its NUL
template <int L, int POS, int BEGIN>
BP_HD auto merlin_head(uint64_t (&a)[25], Cur<POS, BEGIN> c, const char (&label)[L], uint32_t len) {
  auto c1 = strobe_begin_op<STROBE_M | STROBE_A>(a, c);
  auto c2 = strobe_absorb<L - 1>(a, c1, [&](auto i) { return (uint8_t)label[decltype(i)::value]; });
  return strobe_absorb<4>(a, c2, [&](auto i) { return (uint8_t)(len >> (8 * decltype(i)::value)); });
}
// append_message(label, N bytes given as little-endian 32-bit words)
template <int N, int L, int POS, int BEGIN>
BP_HD auto merlin_append_words(uint64_t (&a)[25], Cur<POS, BEGIN> c, const char (&label)[L], const uint32_t* src) {
  uint32_t w[N / 4];                                            // read where it is used: the record never sits in registers as a whole
#pragma unroll
  for (int i = 0; i < N / 4; i++) w[i] = src[i];
  auto c1 = merlin_head(a, c, label, (uint32_t)N);
  auto c2 = strobe_begin_op<STROBE_A>(a, c1);
  return strobe_absorb<N>(a, c2, [&](auto i) { return (uint8_t)(w[decltype(i)::value >> 2] >> (8 * (decltype(i)::value & 3))); });
}
template <int L, int POS, int BEGIN>
BP_HD auto merlin_append_label(uint64_t (&a)[25], Cur<POS, BEGIN> c, const char (&label)[L], const char (&msg)[6]) {
  auto c1 = merlin_head(a, c, label, 5u);
  auto c2 = strobe_begin_op<STROBE_A>(a, c1);
  return strobe_absorb<5>(a, c2, [&](auto i) { return (uint8_t)msg[decltype(i)::value]; });
}
// challenge_bytes(label, 32): the PRF begins with a forced permutation, so the 32 bytes are lanes 0..3 and the cursor ends at (32, 0)
template <int L, int POS, int BEGIN>
BP_HD Cur<32, 0> merlin_challenge32(uint64_t (&a)[25], Cur<POS, BEGIN> c, const char (&label)[L], fr_t& out) {
  auto c1 = merlin_head(a, c, label, 32u);
  auto c2 = strobe_begin_op<STROBE_I | STROBE_A | STROBE_C>(a, c1);
  static_assert(decltype(c2)::pos == 0 && decltype(c2)::begin == 0, "the PRF starts on a fresh block");
#pragma unroll
  for (int i = 0; i < 4; i++) {
    out.l[2 * i] = (uint32_t)a[i];
    out.l[2 * i + 1] = (uint32_t)(a[i] >> 32);
    a[i] = 0;
  }
  return {};
}
// get_and_append_challenge (transcript.rs:70-82): canonical value in `out`, cursor after the re-absorption; *draws counts the draws
template <int L, int POS, int BEGIN>
BP_HD auto plonk_challenge(uint64_t (&a)[25], Cur<POS, BEGIN> c, const char (&label)[L], fr_t& out, uint32_t* draws) {
  auto ok = [](const fr_t& v) {
    fr_t t;
    return big_sub(t, v, Fr::modulus()) != 0 && !big_is_zero(v);
  };
  Cur<32, 0> c1 = merlin_challenge32(a, c, label, out);
  uint32_t k = 1;
  while (!ok(out)) {
    c1 = merlin_challenge32(a, c1, label, out);
    k++;
  }
  if (draws) *draws += k;
  return merlin_append_words<32>(a, c1, label, out.l);
}

// compute_challengs (verifier.rs:193-209) of one 624-byte record given as its 156 little-endian words.  out[0..5] = beta gamma
// alpha zeta nu mu, canonical (NOT Montgomery).  draws (may be null): total number of challenge_bytes calls.
BP_HD void plonk_challenges(const uint32_t* rec, fr_t out[6], uint32_t* draws) {
  uint64_t a[25];
#pragma unroll
  for (int i = 0; i < 25; i++) a[i] = 0;
  {                                                             // Strobe128::new: 1, R + 2, 1, 0, 1, 96, "STROBEv1.0.2"
    const uint8_t head[18] = {1, STROBE_R + 2, 1, 0, 1, 96, 'S', 'T', 'R', 'O', 'B', 'E', 'v', '1', '.', '0', '.', '2'};
#pragma unroll
    for (int i = 0; i < 18; i++) a[i >> 3] ^= (uint64_t)head[i] << (8 * (i & 7));
    keccak_f1600_regs(a);
  }
  auto c0 = strobe_begin_op<STROBE_M | STROBE_A>(a, Cur<0, 0>{});
  auto c1 = strobe_absorb<11>(a, c0, [&](auto i) { return (uint8_t)"Merlin v1.0"[decltype(i)::value]; });
  auto c2 = merlin_append_label(a, c1, "dom-sep", "plonk");
  const uint32_t* ev = rec + 108;                               // the six evaluations behind the nine points
  auto r1a = merlin_append_words<48>(a, c2, "a_1", rec);
  auto r1b = merlin_append_words<48>(a, r1a, "b_1", rec + 12);
  auto r1c = merlin_append_words<48>(a, r1b, "c_1", rec + 24);
  auto r1d = plonk_challenge(a, r1c, "beta", out[0], draws);
  auto r1e = plonk_challenge(a, r1d, "gamma", out[1], draws);
  auto r2a = merlin_append_words<48>(a, r1e, "z_1", rec + 36);
  auto r2b = plonk_challenge(a, r2a, "z_1", out[2], draws);      // alpha is drawn under "z_1" (transcript.rs:24)
  auto r3a = merlin_append_words<48>(a, r2b, "t_lo_1", rec + 48);
  auto r3b = merlin_append_words<48>(a, r3a, "t_mid_1", rec + 60);
  auto r3c = merlin_append_words<48>(a, r3b, "t_hi_1", rec + 72);
  auto r3d = plonk_challenge(a, r3c, "zeta", out[3], draws);
  auto r4a = merlin_append_words<32>(a, r3d, "a_eval", ev);
  auto r4b = merlin_append_words<32>(a, r4a, "b_eval", ev + 8);
  auto r4c = merlin_append_words<32>(a, r4b, "c_eval", ev + 16);
  auto r4d = merlin_append_words<32>(a, r4c, "s1_eval", ev + 24);
  auto r4e = merlin_append_words<32>(a, r4d, "s2_eval", ev + 32);
  auto r4f = merlin_append_words<32>(a, r4e, "z_shifted_eval", ev + 40);
  auto r4g = plonk_challenge(a, r4f, "nu", out[4], draws);
  auto r5a = merlin_append_words<48>(a, r4g, "w_zeta_1", rec + 84);
  auto r5b = merlin_append_words<48>(a, r5a, "w_zeta_omega_1", rec + 96);
  (void)plonk_challenge(a, r5b, "mu", out[5], draws);
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------- kernels
// status word of the scalar checks: the host sets it to ~0; a failing lane does one atomicMin of (proof << 4) | field
// (0..5: that evaluation >= q, 6: a public input, 7: the weight, 8: a given challenge)
constexpr uint32_t VERIFY_BAD_PUBLIC = 6, VERIFY_BAD_WEIGHT = 7, VERIFY_BAD_CHALLENGE = 8;

__device__ __forceinline__ void verify_load_words(uint32_t* dst, const uint8_t* src, int n16) {
  const uint4* q = reinterpret_cast<const uint4*>(src);
  for (int j = 0; j < n16; j++) {
    const uint4 v = q[j];
    dst[4 * j] = v.x; dst[4 * j + 1] = v.y; dst[4 * j + 2] = v.z; dst[4 * j + 3] = v.w;
  }
}
// a scalar in scalar_fmt -> Montgomery; false when canonical bytes are >= q
__device__ __forceinline__ bool verify_load_fr(fr_t& out, const fr_t* p, int fmt) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 lo = q[0], hi = q[1];
  fr_t v;
  v.l[0] = lo.x; v.l[1] = lo.y; v.l[2] = lo.z; v.l[3] = lo.w;
  v.l[4] = hi.x; v.l[5] = hi.y; v.l[6] = hi.z; v.l[7] = hi.w;
  if (fmt == BP_FR_MONT) {
    out = v;
    return true;
  }
  fr_t t;
  const bool ok = big_sub(t, v, Fr::modulus()) != 0;
  Fr::to_mont(out, v);
  return ok;
}

// proofs: m records of 624 bytes (16-byte aligned: 624 = 39 x 16).  chal: m x 6 Montgomery scalars, row j = beta gamma alpha zeta nu mu.
__global__ void __launch_bounds__(64) verify_transcript(const uint8_t* __restrict__ proofs, size_t m, fr_t* __restrict__ chal) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  fr_t c[6];
  plonk_challenges(reinterpret_cast<const uint32_t*>(proofs + (size_t)VERIFY_RECORD_BYTES * j), c, nullptr);
#pragma unroll
  for (int k = 0; k < 6; k++) {
    fr_t t;
    Fr::to_mont(t, c[k]);
    uint4* dst = reinterpret_cast<uint4*>(chal + 6 * j + k);
    dst[0] = make_uint4(t.l[0], t.l[1], t.l[2], t.l[3]);
    dst[1] = make_uint4(t.l[4], t.l[5], t.l[6], t.l[7]);
  }
}

// comp[(k m + j) * 48 ..] = point k of proof j: the order the decoder, the subgroup check and both MSMs walk
__global__ void __launch_bounds__(256) verify_gather(const uint8_t* __restrict__ proofs, size_t m, uint8_t* __restrict__ comp) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)VERIFY_POINTS * m) return;
  const size_t k = t / m, j = t - k * m;
  const uint4* src = reinterpret_cast<const uint4*>(proofs + (size_t)VERIFY_RECORD_BYTES * j + 48 * k);
  uint4* dst = reinterpret_cast<uint4*>(comp + 48 * t);
  dst[0] = src[0];
  dst[1] = src[1];
  dst[2] = src[2];
}

struct VerifyParams {
  fr_t omega, n_inv;          // root_of_unity(n), 1 / n (Montgomery)
  uint32_t log_n;
  int fmt;                    // scalar_fmt of public inputs, weights and given challenges
  int chal_fmt;               // BP_FR_MONT for derived challenges, fmt for given ones
  size_t n_public;
};

__device__ __forceinline__ void verify_store_fr(fr_t* p, const fr_t& v) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

// One proof per lane: verifier.rs:86-191 as scalars.  Outputs, all times the proof's weight rho:
//   scal_b[k m + j], k < 9 : coefficient of proof point k in B        scal_a[j], scal_a[m + j] : rho, rho mu (W_zeta, W_zeta_omega in A)
//   shared[k m + j], k < 9 : the proof's contribution to the scalar of QL QR QM QO QC S1 S2 S3 G
__global__ void __launch_bounds__(128) verify_scalars(const uint8_t* __restrict__ proofs, size_t m, const fr_t* __restrict__ chal,
                                                       const fr_t* __restrict__ weights, const fr_t* __restrict__ publics, VerifyParams P,
                                                       fr_t* __restrict__ scal_b, fr_t* __restrict__ scal_a, fr_t* __restrict__ shared,
                                                       unsigned long long* __restrict__ status) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  unsigned long long bad = ~0ull;
  auto report = [&](uint32_t field) {
    const unsigned long long w = ((unsigned long long)j << 4) | field;
    bad = w < bad ? w : bad;
  };
  fr_t ev[6];                                                   // a b c s1 s2 zw
#pragma unroll
  for (int k = 0; k < 6; k++)
    if (!verify_load_fr(ev[k], reinterpret_cast<const fr_t*>(proofs + (size_t)VERIFY_RECORD_BYTES * j + 432 + 32 * k), BP_FR_BYTES_LE)) report(k);
  fr_t ch[6];                                                   // beta gamma alpha zeta nu mu
#pragma unroll
  for (int k = 0; k < 6; k++)
    if (!verify_load_fr(ch[k], chal + 6 * j + k, P.chal_fmt)) report(VERIFY_BAD_CHALLENGE);
  fr_t rho = Fr::one();
  if (weights && !verify_load_fr(rho, weights + j, P.fmt)) report(VERIFY_BAD_WEIGHT);
  const fr_t &a = ev[0], &b = ev[1], &c = ev[2], &s1 = ev[3], &s2 = ev[4], &zw = ev[5];
  const fr_t &beta = ch[0], &gamma = ch[1], &alpha = ch[2], &zeta = ch[3], &nu = ch[4], &mu = ch[5];
  const fr_t one = Fr::one();

  fr_t zn = zeta;                                               // zeta^n, Z = zeta^n - 1 (verifier.rs:86)
  for (uint32_t k = 0; k < P.log_n; k++) Fr::sqr(zn, zn);
  fr_t Z;
  Fr::sub(Z, zn, one);

  // L_1(zeta) and PI(zeta) = sum_i (-x_i) L_i(zeta), L_i(zeta) = w^i Z / (n (zeta - w^i))  (verifier.rs:89-104).  Z = 0 exactly
  // when zeta is one of the roots, and then L_i(zeta) = [zeta == w^i]; otherwise no denominator vanishes.  The sum of fractions
  // sum_i t_i / d_i is carried as ONE fraction N / D (three products per term) and shares its inversion with 1 / (zeta - 1).
  fr_t l1 = Fr::zero(), pi = Fr::zero();
  const fr_t* row = publics + j * P.n_public;
  if (big_is_zero(Z)) {
    fr_t wi = one;
    if (big_eq(zeta, one)) l1 = one;
    for (size_t i = 0; i < P.n_public; i++) {
      fr_t x;
      if (!verify_load_fr(x, row + i, P.fmt)) report(VERIFY_BAD_PUBLIC);
      if (big_eq(zeta, wi)) Fr::neg(pi, x);
      Fr::mul(wi, wi, P.omega);
    }
  } else {
    fr_t N = Fr::zero(), D = one, wi = one, e;
    Fr::sub(e, zeta, one);
    for (size_t i = 0; i < P.n_public; i++) {
      fr_t x, d, t;
      if (!verify_load_fr(x, row + i, P.fmt)) report(VERIFY_BAD_PUBLIC);
      Fr::sub(d, zeta, wi);
      Fr::mul(t, x, wi);                                        // the numerator is -x_i w^i: the sign goes on at the end
      Fr::mul(N, N, d);
      Fr::mul(t, t, D);
      Fr::add(N, N, t);
      Fr::mul(D, D, d);
      Fr::mul(wi, wi, P.omega);
    }
    fr_t inv, zn_over_n, t;
    Fr::mul(t, D, e);
    fr_invert(inv, t);                                          // 1 / (D (zeta - 1))
    Fr::mul(zn_over_n, Z, P.n_inv);
    Fr::mul(l1, inv, D);                                        // 1 / (zeta - 1)
    Fr::mul(l1, l1, zn_over_n);
    Fr::mul(t, inv, e);                                         // 1 / D
    Fr::mul(t, t, N);
    Fr::mul(t, t, zn_over_n);
    Fr::neg(pi, t);
  }

  fr_t nu2, nu3, nu4, nu5, alpha2, t, u, v;
  Fr::sqr(nu2, nu);
  Fr::mul(nu3, nu2, nu);
  Fr::mul(nu4, nu3, nu);
  Fr::mul(nu5, nu4, nu);
  Fr::sqr(alpha2, alpha);
  auto rl = [&](fr_t& r, const fr_t& s, const fr_t& o) {         // s + o beta + gamma (utils.rs Rlc)
    fr_t p;
    Fr::mul(p, o, beta);
    Fr::add(p, p, s);
    Fr::add(r, p, gamma);
  };
  fr_t l1a2;
  Fr::mul(l1a2, l1, alpha2);
  // z_1: rl(a, zeta) rl(b, k1 zeta) rl(c, k2 zeta) alpha + L_1 alpha^2 + mu, k1 = 2, k2 = 3 (verifier.rs:137-143, 76-77)
  fr_t z2, z3, cz;
  Fr::dbl(z2, zeta);
  Fr::add(z3, z2, zeta);
  rl(t, a, zeta);
  rl(u, b, z2);
  rl(v, c, z3);
  Fr::mul(cz, t, u);
  Fr::mul(cz, cz, v);
  Fr::mul(cz, cz, alpha);
  Fr::add(cz, cz, l1a2);
  Fr::add(cz, cz, mu);
  // perm = rl(a, s1) rl(b, s2) alpha zw: S3 gets -perm beta (:144-149), r_0 gets -perm (c + gamma) (:114-120)
  fr_t perm, cs3, r0;
  rl(t, a, s1);
  rl(u, b, s2);
  Fr::mul(perm, t, u);
  Fr::mul(perm, perm, alpha);
  Fr::mul(perm, perm, zw);
  Fr::mul(cs3, perm, beta);
  Fr::neg(cs3, cs3);
  Fr::add(t, c, gamma);
  Fr::mul(t, t, perm);
  Fr::sub(r0, pi, l1a2);
  Fr::sub(r0, r0, t);
  // G: -(nu a + nu^2 b + nu^3 c + nu^4 s1 + nu^5 s2 + mu zw - r_0)  (:172-179)
  fr_t cg;
  Fr::mul(cg, nu, a);
  Fr::mul(t, nu2, b);
  Fr::add(cg, cg, t);
  Fr::mul(t, nu3, c);
  Fr::add(cg, cg, t);
  Fr::mul(t, nu4, s1);
  Fr::add(cg, cg, t);
  Fr::mul(t, nu5, s2);
  Fr::add(cg, cg, t);
  Fr::mul(t, mu, zw);
  Fr::add(cg, cg, t);
  Fr::sub(cg, r0, cg);
  // t_lo, t_mid, t_hi: -Z, -Z zeta^n, -Z zeta^2n (:150-153)
  fr_t tl, tm, th;
  Fr::neg(tl, Z);
  Fr::mul(tm, tl, zn);
  Fr::mul(th, tm, zn);

  auto put = [&](fr_t* base, int k, const fr_t& coeff) {
    fr_t r;
    Fr::mul(r, coeff, rho);
    verify_store_fr(base + (size_t)k * m + j, r);
  };
  put(scal_b, 0, nu);
  put(scal_b, 1, nu2);
  put(scal_b, 2, nu3);
  put(scal_b, 3, cz);
  put(scal_b, 4, tl);
  put(scal_b, 5, tm);
  put(scal_b, 6, th);
  put(scal_b, 7, zeta);                                         // (:187-191)
  Fr::mul(t, mu, zeta);
  Fr::mul(t, t, P.omega);
  put(scal_b, 8, t);
  put(scal_a, 0, one);
  put(scal_a, 1, mu);
  Fr::mul(t, a, b);
  put(shared, 0, a);                                            // QL QR QM QO QC (:136)
  put(shared, 1, b);
  put(shared, 2, t);
  put(shared, 3, c);
  put(shared, 4, one);
  put(shared, 5, nu4);                                          // S1 S2 (:168-169)
  put(shared, 6, nu5);
  put(shared, 7, cs3);
  put(shared, 8, cg);
  if (bad != ~0ull) atomicMin(status, bad);
}

// out[k] = sum_j shared[k m + j]: block k, 256 lanes striding over the batch, then a tree in LDS
__global__ void __launch_bounds__(256) verify_shared_sum(const fr_t* __restrict__ shared, size_t m, fr_t* __restrict__ out) {
  __shared__ uint32_t part[256 * 8];
  const fr_t* col = shared + (size_t)blockIdx.x * m;
  fr_t acc = Fr::zero();
  for (size_t j = threadIdx.x; j < m; j += 256) {
    fr_t v;
    (void)verify_load_fr(v, col + j, BP_FR_MONT);
    Fr::add(acc, acc, v);
  }
#pragma unroll
  for (int i = 0; i < 8; i++) part[i * 256 + threadIdx.x] = acc.l[i];
  __syncthreads();
  for (uint32_t s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      fr_t v;
#pragma unroll
      for (int i = 0; i < 8; i++) v.l[i] = part[i * 256 + threadIdx.x + s];
      Fr::add(acc, acc, v);
#pragma unroll
      for (int i = 0; i < 8; i++) part[i * 256 + threadIdx.x] = acc.l[i];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) verify_store_fr(out + blockIdx.x, acc);
}
#endif  // __HIPCC__

}  // namespace bp

// g1_ntt.hpp -- the inverse number-theoretic transform over G1: L = i_ntt_381(P_0 .. P_{n-1}) (utils.rs:106-129: omega =
// root_of_unity(n), the 1/n factor, natural order in and out) with G1 additions and scalar multiplications in place of the Fr ones.
// It turns the powers-of-tau SRS into the Lagrange-basis SRS [L_i(tau)] G without knowing tau.  __host__ __device__ lines: the
// kernel (srs_kernels.hpp: g1_ntt_pass) and the host loop below (g1_ntt_host, what tests/test_g1_ntt_host.py runs) execute the same
// schedule, the same butterfly and the same scalar multiplication.
//
// Structure: decimation in time.  Pass s = 0 .. log_n - 1 combines, for every butterfly b < n / 2, the two points at i0 and
// i1 = i0 + 2^s:  (u, v) -> (u + w v, u - w v),  w = omega_n^e.  Pass 0 reads the affine input at the bit-reversed indices (the
// reordering), lifts it with g1_from_affine and scales it by n^-1 (one scalar for every lane); its twiddles are all 1.
// g1_ntt_step is the ONE place that says which butterfly touches which points with which twiddle.
#pragma once
#include "g1.hpp"

namespace bp {

constexpr uint32_t G1_NTT_MAX_LOG = 24;

// Butterfly b of pass s of a transform of n = 2^log_n points (log_n >= 1, s < log_n, b < n / 2): the two slots and the exponent e in
// [0, n) of its twiddle omega_n^e (omega_n = root_of_unity(n); the inverse transform's omega_n^-k is omega_n^(n-k)).
// Lane order: the n / 2^(s+1) butterflies that share one twiddle are neighbours (b = j * groups + g), so that in every pass with at
// least 64 groups all lanes of a wave multiply by the same scalar and the branch on a twiddle bit does not diverge.
struct G1NttStep {
  uint64_t i0, i1, e;
};
BP_HD G1NttStep g1_ntt_step(uint32_t log_n, uint32_t s, uint64_t b) {
  const uint32_t gl = log_n - s - 1;                           // log2 of the groups of pass s
  const uint64_t j = b >> gl, g = b & (((uint64_t)1 << gl) - 1);
  G1NttStep st;
  st.i0 = (g << (s + 1)) | j;
  st.i1 = st.i0 + ((uint64_t)1 << s);
  st.e = j ? ((uint64_t)1 << log_n) - (j << gl) : 0;           // omega_(2^(s+1))^-j
  return st;
}
BP_HD uint64_t g1_ntt_bitrev(uint64_t i, uint32_t log_n) {
  uint64_t r = 0;
  for (uint32_t k = 0; k < log_n; k++) r |= ((i >> k) & 1) << (log_n - 1 - k);
  return r;
}

// r = k p for a canonical scalar k < q < 2^255, variable time (SRS points and twiddles are public): 255 doublings and one addition
// per set bit.  The scalar is shifted through its top limb, so no limb is indexed by a loop variable (registers, not scratch), and the
// loop is kept rolled: one copy of the two formulas in the instruction stream.  r may alias p.
BP_HD void g1_ntt_mul(g1_proj& r, const g1_proj& p, const fr_t& k) {
  fr_t sh;
#pragma unroll
  for (int i = 7; i > 0; i--) sh.l[i] = (k.l[i] << 1) | (k.l[i - 1] >> 31);      // bit 254 to the top
  sh.l[0] = k.l[0] << 1;
  g1_proj acc = g1_identity();
#pragma unroll 1
  for (int i = 0; i < 255; i++) {
    g1_double(acc, acc);
    if (sh.l[7] >> 31) g1_add(acc, acc, p);
#pragma unroll
    for (int t = 7; t > 0; t--) sh.l[t] = (sh.l[t] << 1) | (sh.l[t - 1] >> 31);
    sh.l[0] <<= 1;
  }
  r = acc;
}

// v <- omega_n^e v.  tw[k] = omega_n^k, k < n / 2, Montgomery; omega_n^(n/2) = -1 folds the upper half onto the lower one, and
// the twiddles 1 and -1 (k = 0) cost no scalar multiplication.
BP_HD void g1_ntt_twiddle(g1_proj& v, uint64_t e, uint32_t log_n, const fr_t* tw) {
  const uint64_t half = (uint64_t)1 << (log_n - 1);
  const bool neg = e >= half;
  const uint64_t k = neg ? e - half : e;
  if (k) {
    fr_t w;
    Fr::from_mont(w, tw[k]);
    g1_ntt_mul(v, v, w);
  }
  if (neg) Fp::neg(v.y, v.y);
}
// (u, wv) -> (u + wv, u - wv) by the complete addition: identity operands, u == wv (a doubling) and u == -wv need no case of their own
BP_HD void g1_ntt_butterfly(g1_proj& u, g1_proj& wv) {
  g1_proj m = wv, a;
  Fp::neg(m.y, wv.y);
  g1_add(a, u, wv);
  g1_add(wv, u, m);
  u = a;
}

// Butterfly b of pass s, whole: pass 0 (FIRST) reads `in` (affine, natural order) and writes dst; every other pass reads src.
// n_inv: n^-1 mod q, canonical.
template <bool FIRST>
BP_HD void g1_ntt_pass_at(uint32_t log_n, uint32_t s, uint64_t b, const g1_affine* in, const g1_proj* src, g1_proj* dst, const fr_t* tw,
                          const fr_t& n_inv) {
  const G1NttStep st = g1_ntt_step(log_n, s, b);
  g1_proj u, v;
  if (FIRST) {
    v = g1_from_affine(in[g1_ntt_bitrev(st.i1, log_n)]);
    g1_ntt_mul(v, v, n_inv);
    u = g1_from_affine(in[g1_ntt_bitrev(st.i0, log_n)]);
    g1_ntt_mul(u, u, n_inv);
  } else {
    v = src[st.i1];
  }
  g1_ntt_twiddle(v, st.e, log_n, tw);
  if (!FIRST) u = src[st.i0];
  g1_ntt_butterfly(u, v);
  dst[st.i0] = u;
  dst[st.i1] = v;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The whole transform on the host: what g1_ntt_run (srs.hip) enqueues, pass by pass.  a, b: two buffers of n points; tw and n_inv as
// above.  Returns the buffer that holds the result (natural order, projective).
inline g1_proj* g1_ntt_host(const g1_affine* in, uint32_t log_n, const fr_t* tw, const fr_t& n_inv, g1_proj* a, g1_proj* b) {
  if (log_n == 0) {
    a[0] = g1_from_affine(in[0]);
    return a;
  }
  const uint64_t half = (uint64_t)1 << (log_n - 1);
  g1_proj *src = b, *dst = a;
  for (uint32_t s = 0; s < log_n; s++) {
    for (uint64_t bf = 0; bf < half; bf++) {
      if (s == 0) g1_ntt_pass_at<true>(log_n, s, bf, in, nullptr, dst, tw, n_inv);
      else g1_ntt_pass_at<false>(log_n, s, bf, nullptr, src, dst, tw, n_inv);
    }
    g1_proj* t = src;
    src = dst;
    dst = t;
  }
  return src;
}
#endif

}  // namespace bp

// kzg_open_all.hpp -- all n = 2^log_n KZG proofs of one polynomial f on its domain (Feist, Khovratovich): pi_i opens f at omega_n^i.
// With h_m = sum_{k=0}^{n-2-m} f_{m+1+k} P_k (m <= n - 2, h_{n-1} = 0) the proofs are the forward DFT pi_i = sum_m omega_n^(i m) h_m
// over G1, and h is ONE cyclic convolution of length N = 2n:
//   S^_j = P_{n-2-j} for j <= n - 2, the identity for n - 1 <= j < N      (the first n - 1 SRS points, reversed)
//   c^_t = f_{(t + n - 1) mod N} where that index is < n, else 0
//   h_m  = ( IDFT_N( DFT_N(S^) o DFT_N(c^) ) )_m  for m < n;  entries n .. N - 1 of the inverse transform are NOT zero and are dropped.
// The map is linear in the points: it holds for any point set P_k, powers of tau or not.
//
// Three transforms over G1, all on the schedule, the butterfly and the multiplication of g1_ntt.hpp (decimation in time, pass 0
// reads at the bit-reversed index, twiddles omega^-j: the INVERSE transform without its n^-1):
//   table    : DFT_N(S^), affine, kept per SRS and log_n.  Forward by reversal: the unscaled inverse schedule over
//              x'_j = x_{(len - j) mod len} is the forward DFT in natural order, so pass 0 gathers S^ at the reversed index.
//   Toeplitz : pass 0 multiplies table entry j by ITS OWN scalar N^-1 DFT_N(c^)_j (the slot where the Lagrange transform multiplies by
//              the one scalar n^-1), the other passes are the inverse transform as it stands: IDFT_N of the pointwise product.
//   final    : the forward DFT of length n over the first n outputs of the Toeplitz transform (projective, read in place by pass 0 at
//              the reversed index), no scaling.
// __host__ __device__ lines: the kernels (srs_kernels.hpp: g1_ntt_table_pass0, g1_ntt_toeplitz_pass0, g1_ntt_final_pass0 and
// g1_ntt_pass<false>) and the host loop at the end (what tests/test_kzg_open_all_host.py runs) execute the same index maps, the same
// butterfly and the same multiplication.
#pragma once
#include "g1_ntt.hpp"

namespace bp {

constexpr uint64_t OPEN_ALL_NONE = ~(uint64_t)0;     // "no source": the identity (S^) or zero (c^)

// S^_j, j < 2n: the index of the SRS point it is, or OPEN_ALL_NONE for the identity
BP_HD uint64_t open_all_shat(uint32_t log_n, uint64_t j) {
  const uint64_t n = (uint64_t)1 << log_n;
  return j + 2 <= n ? n - 2 - j : OPEN_ALL_NONE;
}
// c^_t, t < 2n: the index of the coefficient it is, or OPEN_ALL_NONE for zero
BP_HD uint64_t open_all_chat(uint32_t log_n, uint64_t t) {
  const uint64_t n = (uint64_t)1 << log_n, k = (t + n - 1) & (2 * n - 1);
  return k < n ? k : OPEN_ALL_NONE;
}
// forward by reversal: DFT(x)_i = len IDFT(x)_{(len - i) mod len}; the index whose element stands at place j of the reversed sequence
BP_HD uint64_t open_all_reversed(uint32_t log_len, uint64_t j) {
  const uint64_t len = (uint64_t)1 << log_len;
  return (len - j) & (len - 1);
}
// the natural index that pass 0 of a FORWARD transform of 2^log_len points reads for its slot `slot`
BP_HD uint64_t open_all_forward_source(uint32_t log_len, uint64_t slot) {
  return open_all_reversed(log_len, g1_ntt_bitrev(slot, log_len));
}

// ---- pass 0 of the three transforms: butterfly b < len / 2, all twiddles 1 ---------------------------------------------------------
// table: len = 2n; srs: the first n - 1 points of the SRS (affine), never read past index n - 2
BP_HD g1_proj open_all_table_load(uint32_t log_n, uint64_t slot, const g1_affine* srs) {
  const uint64_t k = open_all_shat(log_n, open_all_forward_source(log_n + 1, slot));
  return k == OPEN_ALL_NONE ? g1_identity() : g1_from_affine(srs[k]);
}
BP_HD void open_all_table_pass0_at(uint32_t log_n, uint64_t b, const g1_affine* srs, g1_proj* dst) {
  const G1NttStep st = g1_ntt_step(log_n + 1, 0, b);
  g1_proj u = open_all_table_load(log_n, st.i0, srs), v = open_all_table_load(log_n, st.i1, srs);
  g1_ntt_butterfly(u, v);
  dst[st.i0] = u;
  dst[st.i1] = v;
}
// Toeplitz: len = 2^log_len = 2n; table: DFT_N(S^), affine, natural order; sc: N^-1 DFT_N(c^), Montgomery, natural order.  A zero
// scalar and an identity entry (0, 0) both give the identity (g1_ntt_mul: the accumulator never leaves it).
BP_HD g1_proj open_all_toeplitz_load(uint32_t log_len, uint64_t slot, const g1_affine* table, const fr_t* sc) {
  const uint64_t j = g1_ntt_bitrev(slot, log_len);
  fr_t k;
  Fr::from_mont(k, sc[j]);
  g1_proj p = g1_from_affine(table[j]);
  g1_ntt_mul(p, p, k);
  return p;
}
BP_HD void open_all_toeplitz_pass0_at(uint32_t log_len, uint64_t b, const g1_affine* table, const fr_t* sc, g1_proj* dst) {
  const G1NttStep st = g1_ntt_step(log_len, 0, b);
  g1_proj v = open_all_toeplitz_load(log_len, st.i1, table, sc);
  g1_proj u = open_all_toeplitz_load(log_len, st.i0, table, sc);
  g1_ntt_butterfly(u, v);
  dst[st.i0] = u;
  dst[st.i1] = v;
}
// final: len = n; h: the Toeplitz transform's output, of which only entries < n are read; dst must not be h
BP_HD void open_all_final_pass0_at(uint32_t log_n, uint64_t b, const g1_proj* h, g1_proj* dst) {
  const G1NttStep st = g1_ntt_step(log_n, 0, b);
  g1_proj u = h[open_all_forward_source(log_n, st.i0)], v = h[open_all_forward_source(log_n, st.i1)];
  g1_ntt_butterfly(u, v);
  dst[st.i0] = u;
  dst[st.i1] = v;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// passes 1 .. log_len - 1 of a transform whose pass 0 wrote `dst`: returns the buffer that holds the result (natural order).
// tw[k] = omega_len^k, k < len / 2, Montgomery.
inline g1_proj* open_all_rest_host(uint32_t log_len, const fr_t* tw, g1_proj* dst, g1_proj* other) {
  const uint64_t half = (uint64_t)1 << (log_len - 1);
  const fr_t unused = Fr::zero();
  g1_proj *src = dst, *out = other;
  for (uint32_t s = 1; s < log_len; s++) {
    for (uint64_t b = 0; b < half; b++) g1_ntt_pass_at<false>(log_len, s, b, nullptr, src, out, tw, unused);
    g1_proj* t = src;
    src = out;
    out = t;
  }
  return src;
}
// DFT_N(S^) on the host: srs = the first n - 1 points; a, b: two buffers of 2n points; tw_big[k] = omega_2n^k, k < n
inline g1_proj* open_all_table_host(uint32_t log_n, const g1_affine* srs, const fr_t* tw_big, g1_proj* a, g1_proj* b) {
  const uint64_t n = (uint64_t)1 << log_n;
  for (uint64_t bf = 0; bf < n; bf++) open_all_table_pass0_at(log_n, bf, srs, a);
  return open_all_rest_host(log_n + 1, tw_big, a, b);
}
// the n proofs (projective, natural order) from the affine table and the scalars N^-1 DFT_N(c^) (Montgomery): what open_all_run
// (srs.hip) enqueues, pass by pass.  a, b: two buffers of 2n points; tw_small[k] = omega_n^k, k < n / 2.  log_n >= 1.
inline g1_proj* open_all_proofs_host(uint32_t log_n, const g1_affine* table, const fr_t* sc, const fr_t* tw_big, const fr_t* tw_small,
                                     g1_proj* a, g1_proj* b) {
  const uint64_t n = (uint64_t)1 << log_n;
  for (uint64_t bf = 0; bf < n; bf++) open_all_toeplitz_pass0_at(log_n + 1, bf, table, sc, a);
  g1_proj* h = open_all_rest_host(log_n + 1, tw_big, a, b);
  g1_proj* o = h == a ? b : a;
  for (uint64_t bf = 0; bf < n / 2; bf++) open_all_final_pass0_at(log_n, bf, h, o);
  return open_all_rest_host(log_n, tw_small, o, h);
}
#endif

}  // namespace bp

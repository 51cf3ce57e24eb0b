// kzg_open_cosets.hpp -- the r = n / l cell proofs of one polynomial f on its domain (the second half of Feist, Khovratovich):
// n = 2^log_n, l = 2^log_l <= n, omega = root_of_unity(n).  Cell k < r is the coset { omega^(k + r j) : j < l }, its vanishing
// polynomial x^l - a_k with a_k = omega^(k l), and its ONE proof pi_k = [q_k(tau)] G with q_k = f div (x^l - a_k).
//   pi_k = sum_{m<r} (omega^l)^(k m) h_m                     the forward DFT of length r over G1, root omega^l = root_of_unity(r)
//   h_m  = sum_{j<l} sum_{u=0}^{r-2-m} f_{(m+1+u) l + j} P_{u l + j}   for m <= r - 2,  h_{r-1} = 0
// For each residue j this is the Toeplitz product of kzg_open_all.hpp with n -> r on the strided sequences f^(j)_t = f_{t l + j} and
// P^(j)_u = P_{u l + j}; the l products are summed.  As transforms, R = 2r:
//   S^(j)_i = P_{(r-2-i) l + j} for i <= r - 2, the identity for r - 1 <= i < R
//   c^(j)_t = f^(j)_{(t + r - 1) mod R} where that index is < r, else 0
//   h_m     = ( IDFT_R( sum_j DFT_R(S^(j)) o DFT_R(c^(j)) ) )_m  for m < r;  entries r .. R - 1 are dropped.
// Only P_0 .. P_{n-l-1} are read.  The map is linear in the points.  For l = 1 every index function below IS open_all_shat /
// open_all_chat, the table is open_all's table and the driver runs open_all's passes: bp_kzg_open_all is the case l = 1.
//
// Layout: the table is the l transforms DFT_R(S^(j)) side by side, entry i of residue j at j R + i: 2n affine points, the bytes of
// open_all's table.  The scalars R^-1 DFT_R(c^(j)) lie the same way (ONE batched Fr transform, batch = l, stride = R).
//
// The passes (l >= 2; every butterfly pass is g1_ntt_pass_at<false> of g1_ntt.hpp):
//   table    : pass 0 gathers S^(j) from the affine SRS at the reversed, bit-reversed index (S^(j) is never materialised); the l
//              transforms run side by side, ONE launch per pass: butterfly id B = j R/2 + b, the sub-transform in its high bits.
//   multiply : the 2n products sc_j[i] T_j[i], TWO per lane and no more: lane B = j R + slot, j < l / 2, forms
//              sc_j[i] T_j[i] + sc_{j+l/2}[i] T_{j+l/2}[i] at i = bitrev(slot) and writes it at row j, place `slot`: n lanes, the
//              rows already in the order pass 0 of the inverse transform reads.  (A lane that walked all l residues of its slot
//              would serialise l x 255 group steps.)
//   halve    : log_l - 1 passes of plain complete additions, row j += row j + rows/2, in place, until one row of R points is left.
//   inverse  : the unscaled inverse transform of length R over that row, passes 0 .. log_R - 1 (pass 0's twiddles are all 1 and its
//              input stands bit-reversed already, so it is g1_ntt_pass_at<false> too).  R^-1 is on the scalars.
//   final    : open_all_final_pass0_at with log_n -> log_r over the first r outputs, then passes 1 .. log_r - 1.
// __host__ __device__ lines: the kernels (srs_kernels.hpp: g1_ntt_cosets_table_pass0, g1_ntt_batch_pass, g1_ntt_cosets_mul_pass,
// g1_ntt_cosets_halve_pass, open_cosets_chat_fill, open_cosets_cell_order) and the host loops at the end (what
// tests/test_kzg_open_cosets_host.py runs) execute the same index maps, the same butterfly and the same multiplication.
#pragma once
#include "kzg_open_all.hpp"

namespace bp {

// S^(j)_i, j < l, i < R: the index of the SRS point it is, or OPEN_ALL_NONE for the identity
BP_HD uint64_t open_cosets_shat(uint32_t log_n, uint32_t log_l, uint64_t j, uint64_t i) {
  const uint64_t r = (uint64_t)1 << (log_n - log_l);
  return i + 2 <= r ? ((r - 2 - i) << log_l) + j : OPEN_ALL_NONE;
}
// c^(j)_t, j < l, t < R: the index of the coefficient it is, or OPEN_ALL_NONE for zero
BP_HD uint64_t open_cosets_chat(uint32_t log_n, uint32_t log_l, uint64_t j, uint64_t t) {
  const uint64_t r = (uint64_t)1 << (log_n - log_l), k = (t + r - 1) & (2 * r - 1);
  return k < r ? (k << log_l) + j : OPEN_ALL_NONE;
}
// the cell layout of the values: place c = k l + j of the output holds f(omega^(k + r j)), the natural index k + r j
BP_HD uint64_t open_cosets_value_source(uint32_t log_n, uint32_t log_l, uint64_t c) {
  const uint64_t k = c >> log_l, j = c & (((uint64_t)1 << log_l) - 1);
  return k + (j << (log_n - log_l));
}

// ---- table: butterfly B < n of pass 0 of the l side-by-side transforms of length R; srs is never read past index n - l - 1 ----------
BP_HD g1_proj open_cosets_table_load(uint32_t log_n, uint32_t log_l, uint64_t j, uint64_t slot, const g1_affine* srs) {
  const uint64_t k = open_cosets_shat(log_n, log_l, j, open_all_forward_source(log_n - log_l + 1, slot));
  return k == OPEN_ALL_NONE ? g1_identity() : g1_from_affine(srs[k]);
}
BP_HD void open_cosets_table_pass0_at(uint32_t log_n, uint32_t log_l, uint64_t B, const g1_affine* srs, g1_proj* dst) {
  const uint32_t log_r = log_n - log_l;                                 // R / 2 = r butterflies per transform
  const uint64_t j = B >> log_r;
  const G1NttStep st = g1_ntt_step(log_r + 1, 0, B & (((uint64_t)1 << log_r) - 1));
  g1_proj u = open_cosets_table_load(log_n, log_l, j, st.i0, srs), v = open_cosets_table_load(log_n, log_l, j, st.i1, srs);
  g1_ntt_butterfly(u, v);
  dst += j << (log_r + 1);
  dst[st.i0] = u;
  dst[st.i1] = v;
}
// butterfly B of pass s of `count` transforms of 2^log_len points that lie side by side in src and dst: B = j 2^(log_len - 1) + b
BP_HD void open_cosets_batch_pass_at(uint32_t log_len, uint32_t s, uint64_t B, const g1_proj* src, g1_proj* dst, const fr_t* tw) {
  const uint64_t off = (B >> (log_len - 1)) << log_len;
  g1_ntt_pass_at<false>(log_len, s, B & (((uint64_t)1 << (log_len - 1)) - 1), nullptr, src + off, dst + off, tw, Fr::zero());
}

// ---- multiply: lane B < n = (l / 2) R; log_l >= 1.  table, sc: 2n entries, residue j at j R; dst: n points, row j at j R -------------
BP_HD g1_proj open_cosets_product(uint64_t at, const g1_affine* table, const fr_t* sc) {
  fr_t k;
  Fr::from_mont(k, sc[at]);
  g1_proj p = g1_from_affine(table[at]);
  g1_ntt_mul(p, p, k);
  return p;
}
BP_HD void open_cosets_mul_at(uint32_t log_n, uint32_t log_l, uint64_t B, const g1_affine* table, const fr_t* sc, g1_proj* dst) {
  const uint32_t log_R = log_n - log_l + 1;
  const uint64_t j = B >> log_R, slot = B & (((uint64_t)1 << log_R) - 1);
  const uint64_t at = (j << log_R) + g1_ntt_bitrev(slot, log_R);       // < n; its partner row j + l / 2 lies n entries on
  const g1_proj p = open_cosets_product(at, table, sc), q = open_cosets_product(at + ((uint64_t)1 << log_n), table, sc);
  g1_proj sum;
  g1_add(sum, p, q);
  dst[B] = sum;
}
// halve: lane B < half (= rows / 2 x R points): buf[B] += buf[B + half], in place (a lane reads and writes its own two places only)
BP_HD void open_cosets_halve_at(uint64_t half, uint64_t B, g1_proj* buf) {
  const g1_proj p = buf[B], q = buf[B + half];
  g1_proj sum;
  g1_add(sum, p, q);
  buf[B] = sum;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// the l transforms DFT_R(S^(j)) on the host, side by side (projective): srs = the first n - l points; a, b: two buffers of 2n
// points; tw_big[k] = omega_R^k, k < r.  log_l < log_n.
inline g1_proj* open_cosets_table_host(uint32_t log_n, uint32_t log_l, const g1_affine* srs, const fr_t* tw_big, g1_proj* a, g1_proj* b) {
  if (log_l == 0) return open_all_table_host(log_n, srs, tw_big, a, b);
  const uint64_t n = (uint64_t)1 << log_n;
  const uint32_t log_R = log_n - log_l + 1;
  for (uint64_t B = 0; B < n; B++) open_cosets_table_pass0_at(log_n, log_l, B, srs, a);
  g1_proj *src = a, *out = b;
  for (uint32_t s = 1; s < log_R; s++) {
    for (uint64_t B = 0; B < n; B++) open_cosets_batch_pass_at(log_R, s, B, src, out, tw_big);
    g1_proj* t = src;
    src = out;
    out = t;
  }
  return src;
}
// the r proofs (projective, natural order) from the affine table and the scalars R^-1 DFT_R(c^(j)) (Montgomery): what
// open_cosets_proofs_run (srs.hip) enqueues, pass by pass.  a: n points (2n for log_l = 0), b: R points; tw_big[k] = omega_R^k,
// k < r; tw_small[k] = omega_r^k, k < r / 2.  log_l < log_n.
inline g1_proj* open_cosets_proofs_host(uint32_t log_n, uint32_t log_l, const g1_affine* table, const fr_t* sc, const fr_t* tw_big,
                                        const fr_t* tw_small, g1_proj* a, g1_proj* b) {
  if (log_l == 0) return open_all_proofs_host(log_n, table, sc, tw_big, tw_small, a, b);
  const uint64_t n = (uint64_t)1 << log_n;
  const uint32_t log_r = log_n - log_l, log_R = log_r + 1;
  const uint64_t r = (uint64_t)1 << log_r;
  for (uint64_t B = 0; B < n; B++) open_cosets_mul_at(log_n, log_l, B, table, sc, a);
  for (uint64_t half = n >> 1; half >= 2 * r; half >>= 1)
    for (uint64_t B = 0; B < half; B++) open_cosets_halve_at(half, B, a);
  const fr_t unused = Fr::zero();
  g1_proj *src = a, *out = b;
  for (uint32_t s = 0; s < log_R; s++) {
    for (uint64_t bf = 0; bf < r; bf++) g1_ntt_pass_at<false>(log_R, s, bf, nullptr, src, out, tw_big, unused);
    g1_proj* t = src;
    src = out;
    out = t;
  }
  g1_proj *h = src, *o = out;
  for (uint64_t bf = 0; bf < r / 2; bf++) open_all_final_pass0_at(log_r, bf, h, o);
  return open_all_rest_host(log_r, tw_small, o, h);
}
#endif

}  // namespace bp

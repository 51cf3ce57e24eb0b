// kzg_host.hpp -- the host arithmetic of the KZG calls (capi_kzg.hip, kzg.hip): is the opening point on the evaluation domain, the
// scalars of an opening that are O(count), and the scalars of bp_kzg_verify_reduce.  Host-only inline functions over host_codec.hpp; no
// HIP call and no bp_ctx, so tests/test_kzg_host.py compiles this header alone and checks it on the CPU.
#pragma once
#include <stddef.h>

#include "host_codec.hpp"

namespace bp {

// Is z one of the 2^k-th roots of unity w^m (w = root_of_unity(2^k))?  k squarings decide membership (z^(2^k) == 1); the index then
// comes bit by bit from the bottom: with the low t bits divided out, u = w^(m - m_lo) has order dividing 2^(k-t), and bit t of m is
// set iff u^(2^(k-1-t)) = -1.  At most k^2 / 2 squarings in all (k <= 28): microseconds on the host, against a batched inversion
// that one zero denominator would poison for every element.
inline bool kzg_domain_index(const fr_t& z, uint32_t k, uint64_t* m_out) {
  const fr_t one = Fr::one();
  fr_t t = z;
  for (uint32_t i = 0; i < k; i++) Fr::sqr(t, t);
  if (!big_eq(t, one)) return false;
  fr_t w, winv, u = z;
  host_root_of_unity(w, (uint64_t)1 << k);
  fr_invert(winv, w);                                   // w^-(2^t) along the loop
  uint64_t m = 0;
  for (uint32_t b = 0; b < k; b++) {
    t = u;
    for (uint32_t i = 0; i + b + 1 < k; i++) Fr::sqr(t, t);
    if (!big_eq(t, one)) {
      m |= (uint64_t)1 << b;
      Fr::mul(u, u, winv);
    }
    Fr::sqr(winv, winv);
  }
  *m_out = m;
  return true;
}

// nu^0 .. nu^(count-1); nu == nullptr (one polynomial) gives the single 1
inline void kzg_powers(const fr_t* nu, size_t count, fr_t* out) {
  fr_t p = Fr::one();
  for (size_t j = 0; j < count; j++) {
    out[j] = p;
    if (nu) Fr::mul(p, p, *nu);
  }
}
// y_g = sum_j nu^j y_j
inline fr_t kzg_combine(const fr_t* pows, const fr_t* y, size_t count) {
  fr_t acc = Fr::zero(), t;
  for (size_t j = 0; j < count; j++) {
    Fr::mul(t, pows[j], y[j]);
    Fr::add(acc, acc, t);
  }
  return acc;
}
// (z^n - 1) / n for n = 2^k
inline fr_t kzg_barycentric_scale(const fr_t& z, uint32_t k) {
  fr_t t = z, n_inv;
  for (uint32_t i = 0; i < k; i++) Fr::sqr(t, t);
  Fr::sub(t, t, Fr::one());
  fr_invert(n_inv, fr_from_u64((uint64_t)1 << k));
  Fr::mul(t, t, n_inv);
  return t;
}

// The scalars of the batch check of m claims "C_{i,0..count-1} open to y_{i,*} at z_i, combined by nu_i, with proof W_i" under the
// weights r_i (Montgomery inputs; nu == nullptr: count == 1; r == nullptr: every weight 1):
//   A = sum_i a_i W_i                                     a_i = r_i
//   B = sum_ij c_ij C_ij + sum_i w_i W_i + g G            c_ij = r_i nu_i^j,  w_i = r_i z_i,  g = - sum_ij r_i nu_i^j y_ij
// and the batch holds iff pairing(A, x_2) == pairing(B, G2), i.e. iff a . tau = b for the discrete logarithms.
inline void kzg_reduce_scalars(size_t m, size_t count, const fr_t* z, const fr_t* y, const fr_t* nu, const fr_t* r, fr_t* out_c, fr_t* out_w,
                               fr_t* out_a, fr_t* out_g) {
  fr_t g = Fr::zero();
  for (size_t i = 0; i < m; i++) {
    const fr_t ri = r ? r[i] : Fr::one();
    fr_t c = ri, t;
    for (size_t j = 0; j < count; j++) {
      out_c[i * count + j] = c;
      Fr::mul(t, c, y[i * count + j]);
      Fr::add(g, g, t);
      if (nu) Fr::mul(c, c, nu[i]);
    }
    Fr::mul(out_w[i], ri, z[i]);
    out_a[i] = ri;
  }
  Fr::neg(*out_g, g);
}

}  // namespace bp

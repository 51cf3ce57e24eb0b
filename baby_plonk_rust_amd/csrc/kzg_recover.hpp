// kzg_recover.hpp -- a polynomial rebuilt from some of its cells (the first half of a data-availability recovery; the second half,
// coefficients to cells and proofs, is kzg_open_cosets.hpp).  n = 2^log_n, l = 2^log_l <= n, r = n / l, omega = root_of_unity(n),
// omega_r = omega^l.  Cell k < r is the coset { omega^(k + r j) : j < l }, stored in cell order: place k l + j holds f(omega^(k + r j)).
// Given: m distinct cell indices in any order with their m x l values, and a degree bound d (deg f < d, 1 <= d <= m l).  With M the
// r - m missing indices and Z(x) = prod_{k in M} (x^l - omega_r^k), which vanishes exactly on the missing cells:
//   1  two evaluation sets of Z; its coefficients are never formed.  Z takes r distinct values on the domain and r on the shifted one:
//        Z_dom[i] = prod_{k in M} (omega_r^i - omega_r^k)         i < r, zero exactly on M           (Z(omega^t) = Z_dom[t mod r])
//        Z_cos[i] = prod_{k in M} (s^l omega_r^i - omega_r^k)     i < r, s = 7                        (Z(s omega^t) = Z_cos[t mod r])
//      7 generates Fr*, so s^n != 1 for every n <= 2^32: s^l omega_r^i is no r-th root of unity and no Z_cos[i] is zero.
//   2  E[i] = v_{k,j} Z_dom[k] with k = i mod r, j = i div r where cell k is present, else 0: (f Z) on the whole domain.
//      deg(f Z) < d + (r - m) l <= n, so ONE inverse transform of length n gives its coefficients exactly.
//   3  coefficient i times s^i, forward transform: (f Z)(s omega^i); place i times Z_cos[i mod r]^-1 (the r inverses from one batched
//      inversion); inverse transform, times s^-i: g, the interpolant of the present values, deg g < m l.
//   4  the cells agree with SOME polynomial of degree < d exactly when coefficients d .. n - 1 of g are all zero; the lowest non-zero
//      index is reported otherwise.  With m l == d there is no redundancy and NOTHING to check: g is the interpolant of whatever was
//      given, and a wrong value goes unnoticed.
//   5  the first d coefficients are the result.
// m == r: Z = 1, steps 1 and 3 are skipped (one inverse transform and the check).  log_l == log_n: r = 1.
// Step 1 is evaluated directly, 2 r |M| products: hence r <= 2^KZG_RECOVER_MAX_LOG_R (at most 2^33 products).  The walk over the roots
// is cut into slices of at most KZG_RECOVER_WALK roots; a lane keeps one running product per slice and the partial products of the
// slices are multiplied together (kzg_recover_kernels.hpp).
// __host__ __device__ lines: the kernels (kzg_recover_kernels.hpp) and the host loops at the end (what tests/test_kzg_recover_host.py
// runs, with a naive O(n^2) DFT in place of the transforms) execute the same per-lane bodies.
#pragma once
#include <vector>

#include "host_codec.hpp"

namespace bp {

constexpr uint32_t KZG_RECOVER_WALK = 256;               // roots per slice of the walk of step 1 (mirrored in _lib.py)
constexpr uint32_t KZG_RECOVER_MAX_LOG = 24;             // log_n below this, as for the cell proofs
constexpr uint32_t KZG_RECOVER_MAX_LOG_R = 16;           // r <= 2^16: the direct evaluation of step 1
constexpr uint64_t KZG_RECOVER_SHIFT = 7;                // s
constexpr int32_t RECOVER_ABSENT = -1;                   // slot[k] of a missing cell
constexpr uint64_t RECOVER_NO_POSITION = ~(uint64_t)0;

BP_HD uint64_t recover_slices(uint64_t missing) { return (missing + KZG_RECOVER_WALK - 1) / KZG_RECOVER_WALK; }
// the shapes the map is built for; only then do the slot map and the missing list (r entries each) exist
BP_HD bool recover_shape_ok(uint32_t log_n, uint32_t log_l) {
  return log_l <= log_n && log_n < KZG_RECOVER_MAX_LOG && log_n - log_l <= KZG_RECOVER_MAX_LOG_R;
}

struct RecoverPlan {
  int err;                   // BP_OK or the refusal
  uint64_t bad;              // the position in cell_index the refusal names, else RECOVER_NO_POSITION
  uint64_t n_missing;        // |M|
};
// slot[k], k < r: the position of cell k in cell_index, or RECOVER_ABSENT; missing[0 .. n_missing): M, ascending.  Both have r entries
// and are written only where recover_shape_ok (they may be null otherwise).  Refusals, first rule first:
//   an index >= r                            BP_ERR_INVALID_ARG at its position (log_l > log_n: r = 0, every index is too large)
//   a repeated index                         BP_ERR_INVALID_ARG at the position of the second occurrence -- found through the slot map,
//                                            so in a shape that is refused anyway the shape's refusal is what comes back
//   m l < d, d == 0 or d > n                 BP_ERR_LENGTH
//   log_l > log_n                            BP_ERR_INVALID_ARG (reached by no input: then m > 0 fails the first rule and m == 0 the third)
//   log_n >= 24 or r > 2^16                  BP_ERR_TOO_LARGE
BP_HD RecoverPlan recover_plan(const uint32_t* cell_index, uint64_t m, uint32_t log_n, uint32_t log_l, uint64_t d, int32_t* slot, uint32_t* missing) {
  const bool shape = recover_shape_ok(log_n, log_l);
  const uint64_t r = log_l > log_n ? 0 : (log_n - log_l >= 32 ? (uint64_t)1 << 32 : (uint64_t)1 << (log_n - log_l));
  for (uint64_t i = 0; i < m; i++)
    if (cell_index[i] >= r) return {BP_ERR_INVALID_ARG, i, 0};
  if (shape) {
    for (uint64_t k = 0; k < r; k++) slot[k] = RECOVER_ABSENT;
    for (uint64_t i = 0; i < m; i++) {
      if (slot[cell_index[i]] != RECOVER_ABSENT) return {BP_ERR_INVALID_ARG, i, 0};
      slot[cell_index[i]] = (int32_t)i;
    }
  }
  // m l >= d without forming m l: m >= ceil(d / l); beyond 2^63 both sizes saturate
  const uint64_t need = log_l >= 63 ? (d ? 1 : 0) : (d >> log_l) + ((d & (((uint64_t)1 << log_l) - 1)) ? 1 : 0);
  const bool d_above_n = log_n < 64 && d > ((uint64_t)1 << log_n);
  if (d == 0 || d_above_n || m < need) return {BP_ERR_LENGTH, RECOVER_NO_POSITION, 0};
  if (log_l > log_n) return {BP_ERR_INVALID_ARG, RECOVER_NO_POSITION, 0};
  if (!shape) return {BP_ERR_TOO_LARGE, RECOVER_NO_POSITION, 0};
  uint64_t count = 0;
  for (uint64_t k = 0; k < r; k++)
    if (slot[k] == RECOVER_ABSENT) missing[count++] = (uint32_t)k;
  return {BP_OK, RECOVER_NO_POSITION, count};
}

// ---- the per-lane bodies ---------------------------------------------------------------------------------------------------------------
// step 1, one slice: prod_{lo <= k < hi} (x - roots[k]); roots[k] = omega_r^(missing[k]).  lo == hi gives one.
BP_HD fr_t recover_vanishing_partial_at(const fr_t& x, const fr_t* roots, uint64_t lo, uint64_t hi) {
  fr_t acc = Fr::one();
  for (uint64_t k = lo; k < hi; k++) {
    fr_t t;
    Fr::sub(t, x, roots[k]);
    Fr::mul(acc, acc, t);
  }
  return acc;
}
// step 2: E[i], i < n; values: m x l in cell order, row slot[k] is cell k; z_dom == nullptr stands for Z = 1 (nothing missing)
BP_HD fr_t recover_spread_at(uint32_t log_n, uint32_t log_l, uint64_t i, const int32_t* slot, const fr_t* values, const fr_t* z_dom) {
  const uint32_t log_r = log_n - log_l;
  const uint64_t k = i & (((uint64_t)1 << log_r) - 1), j = i >> log_r;
  const int32_t at = slot[k];
  if (at == RECOVER_ABSENT) return Fr::zero();
  fr_t v = values[((uint64_t)at << log_l) + j];
  if (z_dom) Fr::mul(v, v, z_dom[k]);
  return v;
}
// step 3: place i of (f Z)(s omega^i) times Z_cos[i mod r]^-1
BP_HD fr_t recover_divide_at(uint32_t log_r, uint64_t i, const fr_t& v, const fr_t* z_inv) {
  fr_t out;
  Fr::mul(out, v, z_inv[i & (((uint64_t)1 << log_r) - 1)]);
  return out;
}
// step 4: is coefficient i (d <= i < n) of g non-zero?
BP_HD bool recover_high_nonzero_at(const fr_t* g, uint64_t i) { return !big_is_zero(g[i]); }

// the point sets of step 1: s^l, as a Montgomery element
inline fr_t recover_coset_base(uint32_t log_l) { return fr_pow_u64(fr_from_u64(KZG_RECOVER_SHIFT), (uint64_t)1 << log_l); }

#if !defined(__HIP_DEVICE_COMPILE__)
// z[0 .. r) = Z_dom, z[r .. 2r) = Z_cos, slice by slice as the kernel walks them
inline void recover_vanishing_host(uint32_t log_n, uint32_t log_l, const uint32_t* missing, uint64_t n_missing, fr_t* z) {
  const uint64_t r = (uint64_t)1 << (log_n - log_l);
  fr_t omega_r;
  (void)host_root_of_unity(omega_r, r);
  std::vector<fr_t> roots(n_missing ? n_missing : 1);
  for (uint64_t k = 0; k < n_missing; k++) roots[k] = fr_pow_u64(omega_r, missing[k]);
  const fr_t base = recover_coset_base(log_l);
  for (uint64_t set = 0; set < 2; set++)
    for (uint64_t i = 0; i < r; i++) {
      fr_t x = fr_pow_u64(omega_r, i), acc = Fr::one();
      if (set) Fr::mul(x, x, base);
      for (uint64_t s = 0; s < recover_slices(n_missing); s++) {
        const uint64_t lo = s * KZG_RECOVER_WALK, hi = lo + KZG_RECOVER_WALK < n_missing ? lo + KZG_RECOVER_WALK : n_missing;
        Fr::mul(acc, acc, recover_vanishing_partial_at(x, roots.data(), lo, hi));
      }
      z[set * r + i] = acc;
    }
}
// a <- the DFT of a with root w, by the definition (n^2 products); scale is multiplied in (n^-1 for an inverse)
inline void recover_dft_host(std::vector<fr_t>& a, const fr_t& w, const fr_t& scale) {
  const uint64_t n = a.size();
  std::vector<fr_t> pw(n), out(n);
  pw[0] = Fr::one();
  for (uint64_t k = 1; k < n; k++) Fr::mul(pw[k], pw[k - 1], w);
  for (uint64_t i = 0; i < n; i++) {
    fr_t acc = Fr::zero();
    for (uint64_t k = 0; k < n; k++) {
      fr_t t;
      Fr::mul(t, a[k], pw[(i * k) & (n - 1)]);
      Fr::add(acc, acc, t);
    }
    Fr::mul(out[i], acc, scale);
  }
  a = out;
}
// The whole recovery on the host: values are m x l Montgomery elements in cell order.  out: n elements, the coefficients of g (the
// first d are the result).  Returns the plan's refusal, or BP_ERR_ASSERT with the lowest non-zero index >= d in *first_bad, or BP_OK.
inline int recover_host(uint32_t log_n, uint32_t log_l, const uint32_t* cell_index, const fr_t* values, uint64_t m, uint64_t d, fr_t* out,
                        uint64_t* first_bad) {
  const bool shape = recover_shape_ok(log_n, log_l);
  std::vector<int32_t> slot(shape ? (size_t)1 << (log_n - log_l) : 0);
  std::vector<uint32_t> missing(slot.size());
  const RecoverPlan plan = recover_plan(cell_index, m, log_n, log_l, d, slot.data(), missing.data());
  *first_bad = plan.bad;
  if (plan.err != BP_OK) return plan.err;
  const uint64_t n = (uint64_t)1 << log_n, r = n >> log_l;
  fr_t omega, omega_inv, n_inv;
  (void)host_root_of_unity(omega, n);
  fr_invert(omega_inv, omega);
  fr_invert(n_inv, fr_from_u64(n));
  std::vector<fr_t> z(2 * r), e(n);
  if (plan.n_missing) recover_vanishing_host(log_n, log_l, missing.data(), plan.n_missing, z.data());
  for (uint64_t i = 0; i < n; i++) e[i] = recover_spread_at(log_n, log_l, i, slot.data(), values, plan.n_missing ? z.data() : nullptr);
  recover_dft_host(e, omega_inv, n_inv);
  if (plan.n_missing) {
    const fr_t s = fr_from_u64(KZG_RECOVER_SHIFT);
    fr_t s_inv;
    fr_invert(s_inv, s);
    for (uint64_t i = 0; i < n; i++) Fr::mul(e[i], e[i], fr_pow_u64(s, i));
    recover_dft_host(e, omega, Fr::one());
    std::vector<fr_t> z_inv(r);
    for (uint64_t i = 0; i < r; i++) fr_invert(z_inv[i], z[r + i]);
    for (uint64_t i = 0; i < n; i++) e[i] = recover_divide_at(log_n - log_l, i, e[i], z_inv.data());
    recover_dft_host(e, omega_inv, n_inv);
    for (uint64_t i = 0; i < n; i++) Fr::mul(e[i], e[i], fr_pow_u64(s_inv, i));
  }
  for (uint64_t i = 0; i < n; i++) out[i] = e[i];
  for (uint64_t i = d; i < n; i++)
    if (recover_high_nonzero_at(e.data(), i)) {
      *first_bad = i;
      return BP_ERR_ASSERT;
    }
  return BP_OK;
}
#endif

}  // namespace bp

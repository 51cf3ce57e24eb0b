// kzg_kernels.hpp -- device kernels of a KZG opening of up to KZG_MAX_POLYS polynomials at one point z (kzg.hip).
//   Lagrange form (n = 2^k values f_{j,i} = f_j(w^i) per column, never transformed):
//     off the domain   inv_i = 1 / (z - w^i) from prefix and suffix products and ONE inversion, shared by all columns
//                      y_j = (z^n - 1)/n * sum_i f_{j,i} w^i inv_i                  (barycentric formula)
//                      q_i = (g_i - y_g) / (w^i - z) = (y_g - g_i) inv_i            g = sum_j nu^j f_j,  y_g = sum_j nu^j y_j
//     z = w^m          the zero denominator is replaced by one before the inversion; y_j = f_{j,m}; q_i as above for i != m and
//                      q_m = - sum_{i != m} q_i w^(i-m)
//   Monomial form: the nu-weighted sum of columns of different lengths (the values come from poly_eval_many_run, the quotient from
//   poly_div_run's binomial path).
// Every kernel runs 256-lane workgroups; sums go lane -> LDS tree -> one partial per workgroup -> a one-workgroup second pass.
#pragma once
#include "fr_io.hpp"

namespace bp {

constexpr int KZG_MAX_POLYS = 16;
constexpr uint32_t KZG_SUM_BLOCKS = 1024;      // workgroups per column of a sum at the most (grid-stride above)
constexpr size_t KZG_NO_INDEX = ~(size_t)0;    // "z is off the domain"

struct KzgCols {
  const fr_t* c[KZG_MAX_POLYS];
  size_t n[KZG_MAX_POLYS];
  fr_t w[KZG_MAX_POLYS];                       // nu^j; w[0] = 1 is never multiplied by
  uint32_t count;
};

// sum over the 256 lanes of a workgroup; valid on every lane
__device__ __forceinline__ fr_t kzg_block_sum(const fr_t& v, fr_t* buf) {
  buf[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t stride = 128; stride > 0; stride >>= 1) {
    if (threadIdx.x < stride) {
      fr_t a = buf[threadIdx.x], b = buf[threadIdx.x + stride];
      Fr::add(a, a, b);
      buf[threadIdx.x] = a;
    }
    __syncthreads();
  }
  return buf[0];
}
// g_i = sum_j nu^j f_{j,i}, a column shorter than i contributing nothing
__device__ __forceinline__ fr_t kzg_combine_at(const KzgCols& a, size_t i) {
  fr_t g = i < a.n[0] ? load_fr(&a.c[0][i]) : Fr::zero();
  for (uint32_t j = 1; j < a.count; j++) {
    if (i >= a.n[j]) continue;
    fr_t f = load_fr(&a.c[j][i]);
    Fr::mul(f, f, a.w[j]);
    Fr::add(g, g, f);
  }
  return g;
}

// den_i = z - w^i, and one where it would be zero (i == m, z = w^m)
__global__ void __launch_bounds__(256) kzg_lag_denoms(const fr_t* __restrict__ roots, size_t n, fr_t z, size_t m, fr_t* __restrict__ den) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fr_t d = load_fr(&roots[i]);
  Fr::sub(d, z, d);
  store_fr(&den[i], i == m ? Fr::one() : d);
}
// inv_i = (prod_{l<i} den_l) (prod_{l>i} den_l) / prod_l den_l, and winv_i = w^i inv_i
__global__ void __launch_bounds__(256) kzg_lag_invert(const fr_t* __restrict__ pre, const fr_t* __restrict__ suf, const fr_t* __restrict__ roots,
                                                       fr_t total_inv, size_t n, fr_t* __restrict__ inv, fr_t* __restrict__ winv) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fr_t p = load_fr(&pre[i]), s = load_fr(&suf[i]), w = load_fr(&roots[i]);
  Fr::mul(p, p, s);
  Fr::mul(p, p, total_inv);
  store_fr(&inv[i], p);
  Fr::mul(p, p, w);
  store_fr(&winv[i], p);
}
// partial[j * gridDim.x + b] = this workgroup's share of sum_i f_{j,i} winv_i   (j = blockIdx.y)
__global__ void __launch_bounds__(256) kzg_lag_values_partial(KzgCols a, const fr_t* __restrict__ winv, size_t n, fr_t* __restrict__ partial) {
  __shared__ fr_t buf[256];
  const fr_t* __restrict__ f = a.c[blockIdx.y];
  fr_t acc = Fr::zero();
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    fr_t v = load_fr(&f[i]), u = load_fr(&winv[i]);
    Fr::mul(v, v, u);
    Fr::add(acc, acc, v);
  }
  const fr_t s = kzg_block_sum(acc, buf);
  if (threadIdx.x == 0) store_fr(&partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x], s);
}
// out[j] = sum of the `blocks` partials of row j (j = blockIdx.x); negate != 0 stores the negated sum
__global__ void __launch_bounds__(256) kzg_sum_rows(const fr_t* __restrict__ partial, uint32_t blocks, int negate, fr_t* __restrict__ out) {
  __shared__ fr_t buf[256];
  fr_t acc = Fr::zero();
  for (uint32_t b = threadIdx.x; b < blocks; b += blockDim.x) {
    fr_t v = load_fr(&partial[(size_t)blockIdx.x * blocks + b]);
    Fr::add(acc, acc, v);
  }
  fr_t s = kzg_block_sum(acc, buf);
  if (threadIdx.x == 0) {
    if (negate) Fr::neg(s, s);
    store_fr(&out[blockIdx.x], s);
  }
}
// out[j] = f_{j,m}
__global__ void __launch_bounds__(256) kzg_gather_row(KzgCols a, size_t m, fr_t* __restrict__ out) {
  const uint32_t j = threadIdx.x;
  if (j < a.count) store_fr(&out[j], m < a.n[j] ? load_fr(&a.c[j][m]) : Fr::zero());
}
// q_i = (y_g - g_i) inv_i, and zero at i == m
__global__ void __launch_bounds__(256) kzg_lag_quotient(KzgCols a, fr_t y_g, const fr_t* __restrict__ inv, size_t n, size_t m, fr_t* __restrict__ q) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fr_t g = kzg_combine_at(a, i), u = load_fr(&inv[i]);
  Fr::sub(g, y_g, g);
  Fr::mul(g, g, u);
  store_fr(&q[i], i == m ? Fr::zero() : g);
}
// partial[b] = this workgroup's share of sum_i q_i w^(i-m)   (q_m is still zero; n is a power of two)
__global__ void __launch_bounds__(256) kzg_lag_diag_partial(const fr_t* __restrict__ q, const fr_t* __restrict__ roots, size_t n, size_t m,
                                                             fr_t* __restrict__ partial) {
  __shared__ fr_t buf[256];
  fr_t acc = Fr::zero();
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    fr_t v = load_fr(&q[i]), w = load_fr(&roots[(i + n - m) & (n - 1)]);
    Fr::mul(v, v, w);
    Fr::add(acc, acc, v);
  }
  const fr_t s = kzg_block_sum(acc, buf);
  if (threadIdx.x == 0) store_fr(&partial[blockIdx.x], s);
}
// g_i = sum_j nu^j f_{j,i} for i < n (Monomial form: the columns have their own lengths)
__global__ void __launch_bounds__(256) kzg_lincomb(KzgCols a, size_t n, fr_t* __restrict__ g) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  store_fr(&g[i], kzg_combine_at(a, i));
}

// ---- cell claims (bp_kzg_verify_cells_reduce): out[t] = - sum_{i<m} rho_i w_i^t c[i l + t], t < l = 2^log_l ---------------------------
// c: the m rows after their inverse transform of length l (l^-1 included), so that w_i^t c[i l + t] with w_i = omega^(-k_i) is
// coefficient t of the interpolant of claim i on its coset; out: the scalars of P_0 .. P_{l-1} in B.  One lane per t walks the m
// claims (t < 2^24 is one exponent limb): m x ~50 products per lane, l lanes.  Reads c below m l, w and rho below m; writes out below l.
__global__ void __launch_bounds__(256) kzg_cells_combine(const fr_t* __restrict__ c, const fr_t* __restrict__ w, const fr_t* __restrict__ rho, size_t m,
                                                          uint32_t log_l, fr_t* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ((size_t)1 << log_l)) return;
  const uint32_t e[1] = {(uint32_t)t};
  fr_t acc = Fr::zero();
  for (size_t i = 0; i < m; i++) {
    fr_t p, v = load_fr(&c[(i << log_l) + t]);
    Fr::pow(p, load_fr(&w[i]), e, 1);
    Fr::mul(p, p, load_fr(&rho[i]));
    Fr::mul(p, p, v);
    Fr::add(acc, acc, p);
  }
  Fr::neg(acc, acc);
  store_fr(&out[t], acc);
}

}  // namespace bp

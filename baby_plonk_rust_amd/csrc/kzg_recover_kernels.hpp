// kzg_recover_kernels.hpp -- device kernels of bp_kzg_recover (capi_kzg_recover.hip): the per-lane bodies of
// kzg_recover.hpp behind one lane per element.  Every kernel runs 256-lane workgroups.  The transforms, the powers of the shift and the
// batched inversion are the library's (ntt.hip, poly.hip).
//   recover_missing_roots        roots[k] = omega_r^(missing[k]), gathered from the table of the r-th roots of unity
//   recover_vanishing_eval       step 1, the hot kernel: 2 r |M| products.  A workgroup is four waves over the SAME 64 points; wave w
//                                walks slice 4 z + w of the roots (z = blockIdx.z), so every root is loaded at a wave-uniform address
//                                and a lane keeps one running product in registers.  The four partial products of a point meet in LDS.
//                                blockIdx.y selects the point set: 0 the domain (base 1), 1 the shifted domain (base s^l).
//   recover_vanishing_combine    only with more than four slices: the products of the ceil(slices / 4) workgroups of a point
//   recover_spread               step 2: every place of E written once, coalesced; no memset
//   recover_divide               step 3: in place
//   recover_high_nonzero         step 4: atomicMin of the lowest non-zero index >= d into one 64-bit word (all ones: none)
#pragma once
#include "fr_io.hpp"
#include "kzg_recover.hpp"

namespace bp {

constexpr uint32_t RECOVER_WAVES = 4;                    // waves of a workgroup = slices whose products meet in LDS
constexpr uint32_t RECOVER_POINTS = 64;                  // points of a workgroup = lanes of a wave

// workgroups along z of recover_vanishing_eval
inline uint32_t recover_slice_groups(uint64_t n_missing) { return (uint32_t)((recover_slices(n_missing) + RECOVER_WAVES - 1) / RECOVER_WAVES); }

// reads dom below r (missing[k] < r) and missing below n_missing; writes roots below n_missing
__global__ void __launch_bounds__(256) recover_missing_roots(const fr_t* __restrict__ dom, const uint32_t* __restrict__ missing, uint32_t n_missing,
                                                              fr_t* __restrict__ roots) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_missing) return;
  store_fr(&roots[k], load_fr(&dom[missing[k]]));
}

// grid (ceil(r / 64), 2, groups).  out[(set * groups + z) * r + i]: with one group that is Z_dom | Z_cos itself.  Reads dom below r and
// roots below n_missing; a wave whose slice starts at or past n_missing multiplies by one.
__global__ void __launch_bounds__(256) recover_vanishing_eval(const fr_t* __restrict__ dom, uint32_t r, fr_t base, const fr_t* __restrict__ roots,
                                                               uint32_t n_missing, fr_t* __restrict__ out) {
  __shared__ fr_t buf[RECOVER_WAVES][RECOVER_POINTS];
  const uint32_t lane = threadIdx.x & (RECOVER_POINTS - 1);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / RECOVER_POINTS);      // uniform: the loads of the walk are too
  const uint32_t i = blockIdx.x * RECOVER_POINTS + lane;
  const uint64_t slice = (uint64_t)blockIdx.z * RECOVER_WAVES + wave;
  const uint64_t lo = slice * KZG_RECOVER_WALK < n_missing ? slice * KZG_RECOVER_WALK : n_missing;
  const uint64_t hi = lo + KZG_RECOVER_WALK < n_missing ? lo + KZG_RECOVER_WALK : n_missing;
  fr_t p = Fr::one();
  if (i < r) {
    fr_t x = load_fr(&dom[i]);
    if (blockIdx.y) Fr::mul(x, x, base);
    p = recover_vanishing_partial_at(x, roots, lo, hi);
  }
  buf[wave][lane] = p;
  __syncthreads();
  if (wave != 0 || i >= r) return;
  for (uint32_t w = 1; w < RECOVER_WAVES; w++) Fr::mul(p, p, buf[w][lane]);
  store_fr(&out[((size_t)blockIdx.y * gridDim.z + blockIdx.z) * r + i], p);
}

// grid (ceil(r / 256), 2): z[set * r + i] = prod_{g < groups} partial[(set * groups + g) * r + i]
__global__ void __launch_bounds__(256) recover_vanishing_combine(const fr_t* __restrict__ partial, uint32_t r, uint32_t groups, fr_t* __restrict__ z) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r) return;
  const fr_t* __restrict__ row = partial + (size_t)blockIdx.y * groups * r + i;
  fr_t p = load_fr(row);
  for (uint32_t g = 1; g < groups; g++) Fr::mul(p, p, load_fr(row + (size_t)g * r));
  store_fr(&z[(size_t)blockIdx.y * r + i], p);
}

// reads slot below r, values below m l (slot[k] < m), z_dom below r (nullptr: Z = 1); writes out below n.  values and out do not overlap.
__global__ void __launch_bounds__(256) recover_spread(uint32_t log_n, uint32_t log_l, const int32_t* __restrict__ slot, const fr_t* __restrict__ values,
                                                       const fr_t* __restrict__ z_dom, fr_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ((size_t)1 << log_n)) return;
  store_fr(&out[i], recover_spread_at(log_n, log_l, i, slot, values, z_dom));
}

// data[i] *= z_inv[i & (r - 1)], i < n
__global__ void __launch_bounds__(256) recover_divide(uint32_t log_n, uint32_t log_r, const fr_t* __restrict__ z_inv, fr_t* __restrict__ data) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ((size_t)1 << log_n)) return;
  store_fr(&data[i], recover_divide_at(log_r, i, load_fr(&data[i]), z_inv));
}

// lanes over [d, n); *lowest starts as all ones
__global__ void __launch_bounds__(256) recover_high_nonzero(const fr_t* __restrict__ g, size_t d, size_t n, unsigned long long* __restrict__ lowest) {
  const size_t i = d + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (recover_high_nonzero_at(g, i)) atomicMin(lowest, (unsigned long long)i);
}

}  // namespace bp

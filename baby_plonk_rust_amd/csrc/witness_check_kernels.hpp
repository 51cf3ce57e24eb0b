// witness_check_kernels.hpp -- does a witness satisfy a circuit, and if not, where?  (bp_circuit_check_sigma / _witness)
// The reference only panics (prover.rs:319 z_n != 1, :615 r(zeta) != 0); these kernels name the row and the cell.
//   sigma_decode    S1 S2 S3 -> the permutation as cell numbers (sigma_decode.hpp), once per circuit
//   sigma_indegree  is it a permutation?  (every cell the target of exactly one cell)
//   witness_check   the gate equation of every row (prover.rs:370-376) and value(u) == value(sigma(u)) of every cell
// Cells are numbered 3 * row + col.  Findings go to four 64-bit words, the pattern of srs_decode48's status word: a failing lane
// adds one to a counter and does one atomicMin of its position, so one 32-byte read gives the counts and the lowest positions.
#pragma once
#include "fr_io.hpp"
#include "sigma_decode.hpp"

namespace bp {

// Status words, finding kind k = 0 or 1: word k counts, word 2 + k holds the lowest position (the host sets 0 and ~0).
//   bp_circuit_check_sigma:   kind 0 a cell whose value is no label, kind 1 a cell that is the target of != 1 cells; position = the cell
//   bp_circuit_check_witness: kind 0 a row with a non-zero residual (position = the row), kind 1 a cell u whose value differs from
//                             the value at sigma(u) (position = (u << 32) | sigma(u))
__device__ __forceinline__ void check_report(unsigned long long* status, int kind, unsigned long long where) {
  atomicAdd(status + kind, 1ull);
  atomicMin(status + 2 + kind, where);
}

// one lane per cell of lag[5n .. 8n): lane i holds S_(i / n)[i % n]
__global__ void __launch_bounds__(256) sigma_decode(const fr_t* __restrict__ sig, uint32_t log_n, SigmaConsts k, const fr_t* __restrict__ winv,
                                                     uint32_t* __restrict__ target, unsigned long long* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, n = (size_t)1 << log_n;
  if (i >= 3 * n) return;
  const size_t u = 3 * (i & (n - 1)) + (i >> log_n);
  const uint32_t t = sigma_decode_cell(k, winv, load_fr(&sig[i]));
  if (t == SIGMA_NO_CELL) check_report(status, 0, u);
  target[u] = t;
}

// pass 1: count[target[u]]++ (on a permutation every address is hit once); pass 2: cells whose count is not 1
__global__ void __launch_bounds__(256) sigma_indegree_count(const uint32_t* __restrict__ target, size_t cells, uint32_t* __restrict__ count) {
  const size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= cells) return;
  const uint32_t t = target[u];
  if (t < cells) atomicAdd(&count[t], 1u);
}
__global__ void __launch_bounds__(256) sigma_indegree_report(const uint32_t* __restrict__ count, size_t cells, unsigned long long* __restrict__ status) {
  const size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= cells) return;
  if (count[u] != 1) check_report(status, 1, u);
}

// one lane per row.  pi == nullptr: no public inputs.  target: a permutation of the 3n cells (the caller has checked).
__global__ void __launch_bounds__(256) witness_check(const fr_t* __restrict__ a, const fr_t* __restrict__ b, const fr_t* __restrict__ c,
                                                      const fr_t* __restrict__ pi, const fr_t* __restrict__ lag, size_t n,
                                                      const uint32_t* __restrict__ target, unsigned long long* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const fr_t va = load_fr(&a[i]), vb = load_fr(&b[i]), vc = load_fr(&c[i]);
  fr_t r, t;
  Fr::mul(r, load_fr(&lag[i]), va);                              // ql a
  Fr::mul(t, load_fr(&lag[n + i]), vb);                          // qr b
  Fr::add(r, r, t);
  Fr::mul(t, va, vb);
  Fr::mul(t, t, load_fr(&lag[2 * n + i]));                       // qm a b
  Fr::add(r, r, t);
  Fr::mul(t, load_fr(&lag[3 * n + i]), vc);                      // qo c
  Fr::add(r, r, t);
  if (pi) Fr::add(r, r, load_fr(&pi[i]));
  Fr::add(r, r, load_fr(&lag[4 * n + i]));                       // qc
  if (!big_is_zero(r)) check_report(status, 0, i);
#pragma unroll
  for (uint32_t col = 0; col < 3; col++) {
    const size_t u = 3 * i + col;
    const uint32_t v = target[u];
    if (v >= 3 * n) continue;
    const uint32_t vcol = v % 3;
    const fr_t* src = vcol == 0 ? a : vcol == 1 ? b : c;
    const fr_t mine = col == 0 ? va : col == 1 ? vb : vc;
    if (!big_eq(mine, load_fr(&src[v / 3]))) check_report(status, 1, ((unsigned long long)u << 32) | v);
  }
}

}  // namespace bp

// sigma_decode.hpp -- the inverse of Cell::label (utils.rs:28-37): which cell does a value of S1, S2, S3 name?
// Cell (col, row) of a 2^log_n-row circuit carries the label (col + 1) w^row, w = root_of_unity(n), and the sigma columns hold
// labels (program.rs:126-137).  A value s is inverted with Fr arithmetic alone, no table of labels and no sort:
//   column  s^n (log_n squarings) is 1, 2^n or 3^n -- pairwise distinct for every n <= 2^32, since 2, 3 and 3/2 have no order
//           dividing 2^32 -- and anything else is no label; x = s / (col + 1) then lies in <w>, whose order is 2^log_n
//   row     the discrete logarithm of x to the base w bit by bit (Pohlig-Hellman): for j = 0 .. log_n - 1 the power
//           y^(2^(log_n-1-j)) is 1 or -1; -1 sets bit j and y *= w^(-2^j).  log_n (log_n - 1) / 2 squarings, <= log_n products.
// Everything is __host__ __device__ with ONE algorithm on both sides: the CPU test (tests/test_sigma_decode_host.py) compiles
// exactly the code the kernels of witness_check_kernels.hpp run.  Variable time: the circuit is public.
#pragma once
#include "fields.hpp"

namespace bp {

constexpr uint32_t SIGMA_NO_CELL = 0xffffffffu;      // what a value that is no label decodes to
constexpr uint32_t SIGMA_MAX_LOG_N = 24;             // bp_circuit_load's bound: 3 * 2^24 cells fit 32 bits

// Per circuit size, computed once on the host (sigma_consts): k^n and 1 / k for the column numbers k = 1, 2, 3
struct SigmaConsts {
  uint32_t log_n;
  fr_t kn[3];
  fr_t kinv[3];
};
// ... and w^(-2^j), j < log_n.  The decode indexes it with its loop counter, so it lives in memory (HBM on the device), never in a
// register array.
struct SigmaTable {
  fr_t winv[SIGMA_MAX_LOG_N];
};

// Cells are numbered 3 * row + col everywhere (row-major, as bp_make_s_polynomials numbers them).
// -> the cell s is the label of, or SIGMA_NO_CELL.  winv: SigmaTable::winv of the same log_n.
BP_HD uint32_t sigma_decode_cell(const SigmaConsts& k, const fr_t* __restrict__ winv, const fr_t& s) {
  fr_t t;
  if (!big_sub(t, s, Fr::modulus())) return SIGMA_NO_CELL;      // limbs >= q are no Montgomery value at all
  t = s;
#pragma unroll 1
  for (uint32_t i = 0; i < k.log_n; i++) Fr::sqr(t, t);
  uint32_t col = 3;
#pragma unroll
  for (int c = 2; c >= 0; c--) col = big_eq(t, k.kn[c]) ? (uint32_t)c : col;
  if (col == 3) return SIGMA_NO_CELL;
  fr_t kinv = k.kinv[0];
#pragma unroll
  for (int c = 1; c < 3; c++) big_select(kinv, col == (uint32_t)c, k.kinv[c], kinv);
  fr_t y;
  Fr::mul(y, s, kinv);
  const fr_t one = Fr::one();
  uint32_t row = 0;
#pragma unroll 1
  for (uint32_t j = 0; j < k.log_n; j++) {
    t = y;
#pragma unroll 1
    for (uint32_t i = j + 1; i < k.log_n; i++) Fr::sqr(t, t);
    if (!big_eq(t, one)) {                                     // -1: y still has the factor w^(2^j)
      row |= 1u << j;
      Fr::mul(y, y, winv[j]);
    }
  }
  return big_eq(y, one) ? 3 * row + col : SIGMA_NO_CELL;       // y^n = 1 makes every power above +-1, so y ends as 1; checked all the same
}

// ---- host side: the constants, and the loop over a circuit's cells
inline void sigma_consts(uint32_t log_n, SigmaConsts* k, SigmaTable* tbl) {
  k->log_n = log_n;
  fr_t v = Fr::one();
  for (int c = 0; c < 3; c++) {
    fr_t p = v;
    for (uint32_t i = 0; i < log_n; i++) Fr::sqr(p, p);
    k->kn[c] = p;
    fr_invert(k->kinv[c], v);
    Fr::add(v, v, Fr::one());
  }
  fr_t w = fr_root_of_unity(true);                             // 1 / root_of_unity(2^log_n) (utils.rs:39-43): ROOT_OF_UNITY has order 2^32
  for (uint32_t i = log_n; i < 32; i++) Fr::sqr(w, w);
  for (uint32_t j = 0; j < SIGMA_MAX_LOG_N; j++) {
    tbl->winv[j] = j < log_n ? w : Fr::one();
    Fr::sqr(w, w);
  }
}
// the host loop: target[3 * row + col] for the three sigma columns of n = 2^log_n values each; returns how many are no label
inline size_t sigma_decode_host(uint32_t log_n, const fr_t* s1, const fr_t* s2, const fr_t* s3, uint32_t* target) {
  SigmaConsts k;
  SigmaTable tbl;
  sigma_consts(log_n, &k, &tbl);
  const fr_t* s[3] = {s1, s2, s3};
  size_t bad = 0;
  for (size_t row = 0; row < ((size_t)1 << log_n); row++)
    for (int col = 0; col < 3; col++) {
      const uint32_t t = sigma_decode_cell(k, tbl.winv, s[col][row]);
      target[3 * row + col] = t;
      bad += t == SIGMA_NO_CELL;
    }
  return bad;
}

}  // namespace bp

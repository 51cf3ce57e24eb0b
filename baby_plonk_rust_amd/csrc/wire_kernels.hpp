// wire_kernels.hpp -- a circuit from its wire ids (bp_circuit_load_wires) and a witness from a value per variable
// (bp_circuit_assign_device / bp_prove_assignment).  Shapes and rules: wire_plan.hpp.  Cells are numbered 3 * row + col.
//   wire_max_id       the largest id: how many 8-bit passes the sort needs
//   wire_hist         a tile's 256 digit counts -> hist[digit * tiles + tile]
//   wire_scan_chunks  exclusive scan of hist inside chunks of WIRE_SCAN_CHUNK entries, the chunk totals aside
//   wire_scan_sums    exclusive scan of the chunk totals (one workgroup)
//   wire_scatter      keys and cells of a tile to their places, stable: behind every key of the same digit in front of them
//   wire_link         S[cell] = label(pred), sigma_target[cell] = pred from the sorted order; every cell written once, no atomics
//   wire_gather       a b c PI from values[wire id]; an id beyond the values raises the lowest offending cell
// Every kernel runs WIRE_BLOCK = 256 lanes: four waves of 64, ballots are 64 bits wide.
#pragma once
#include "fr_io.hpp"
#include "wire_plan.hpp"

namespace bp {

__device__ __forceinline__ uint32_t wire_wave_scan_incl(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}
// exclusive scan of one value per lane over the 256 lanes of a workgroup; *total: the sum (the same in every lane)
__device__ __forceinline__ uint32_t wire_block_scan_excl(uint32_t v, uint32_t* total) {
  __shared__ uint32_t wave_sum[WIRE_WAVES];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t incl = wire_wave_scan_incl(v, lane);
  __syncthreads();                                              // the previous call's readers are done with wave_sum
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < WIRE_WAVES; w++) {
    const uint32_t s = wave_sum[w];
    before += w < wave ? s : 0;
    all += s;
  }
  *total = all;
  return before + incl - v;
}

__global__ void __launch_bounds__(WIRE_BLOCK) wire_max_id(const uint32_t* __restrict__ ids, size_t cells, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * WIRE_BLOCK + threadIdx.x;
  uint32_t v = i < cells ? ids[i] : 0;
#pragma unroll
  for (uint32_t d = 32; d >= 1; d >>= 1) {
    const uint32_t t = __shfl_xor(v, d, 64);
    v = t > v ? t : v;
  }
  if ((threadIdx.x & 63) == 0 && v) atomicMax(out, v);
}

__global__ void __launch_bounds__(WIRE_BLOCK) wire_hist(const uint32_t* __restrict__ keys, size_t cells, uint32_t pass, uint32_t tiles,
                                                        uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[WIRE_RADIX];
  h[threadIdx.x] = 0;
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * WIRE_TILE;
#pragma unroll
  for (uint32_t r = 0; r < WIRE_ROUNDS; r++) {
    const size_t j = base + (size_t)r * WIRE_BLOCK + threadIdx.x;
    if (j < cells) atomicAdd(&h[wire_digit(keys[j], pass)], 1u);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

__global__ void __launch_bounds__(WIRE_BLOCK) wire_scan_chunks(uint32_t* __restrict__ hist, size_t entries, uint32_t* __restrict__ sums) {
  const size_t e0 = (size_t)blockIdx.x * WIRE_SCAN_CHUNK + (size_t)threadIdx.x * WIRE_SCAN_PER_LANE;
  uint32_t v[WIRE_SCAN_PER_LANE], mine = 0;
#pragma unroll
  for (uint32_t k = 0; k < WIRE_SCAN_PER_LANE; k++) {
    v[k] = e0 + k < entries ? hist[e0 + k] : 0;
    mine += v[k];
  }
  uint32_t total;
  uint32_t run = wire_block_scan_excl(mine, &total);
#pragma unroll
  for (uint32_t k = 0; k < WIRE_SCAN_PER_LANE; k++) {
    if (e0 + k < entries) hist[e0 + k] = run;
    run += v[k];
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums[0 .. m) -> their exclusive scan
__global__ void __launch_bounds__(WIRE_BLOCK) wire_scan_sums(uint32_t* __restrict__ sums, uint32_t m) {
  uint32_t carry = 0;
  for (uint32_t at = 0; at < m; at += WIRE_BLOCK) {
    const uint32_t i = at + threadIdx.x;
    const uint32_t v = i < m ? sums[i] : 0;
    uint32_t total;
    const uint32_t ex = wire_block_scan_excl(v, &total);
    if (i < m) sums[i] = carry + ex;
    carry += total;
  }
}

// i_in == nullptr: the first pass, the payload is the position itself.  Lane t takes keys base + r * 256 + t, r < WIRE_ROUNDS: the
// order inside a tile is (round, wave, lane).  Per round a wave matches equal digits with eight ballots; the lowest lane of a digit
// leaves the wave's count in LDS, lane `digit` turns the 32 (round, wave) counts of its digit into first positions, and a key lands
// at that position plus the count of equal digits on the lanes below it.
__global__ void __launch_bounds__(WIRE_BLOCK) wire_scatter(const uint32_t* __restrict__ k_in, const uint32_t* __restrict__ i_in, size_t cells,
                                                           uint32_t pass, uint32_t tiles, const uint32_t* __restrict__ hist,
                                                           const uint32_t* __restrict__ sums, uint32_t* __restrict__ k_out,
                                                           uint32_t* __restrict__ i_out) {
  __shared__ uint32_t cnt[WIRE_ROUNDS * WIRE_WAVES * WIRE_RADIX];
  static_assert(sizeof(cnt) == WIRE_SCATTER_LDS, "wire_plan.hpp states the LDS of wire_scatter");
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t k = 0; k < WIRE_ROUNDS * WIRE_WAVES; k++) cnt[k * WIRE_RADIX + threadIdx.x] = 0;
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * WIRE_TILE;
  const unsigned long long below = (1ull << lane) - 1;
  uint32_t key[WIRE_ROUNDS], rank[WIRE_ROUNDS];
#pragma unroll
  for (uint32_t r = 0; r < WIRE_ROUNDS; r++) {
    const size_t j = base + (size_t)r * WIRE_BLOCK + threadIdx.x;
    const bool valid = j < cells;
    key[r] = valid ? k_in[j] : 0;
    const uint32_t d = wire_digit(key[r], pass);
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < WIRE_RADIX_BITS; b++) {
      const bool bit = (d >> b) & 1;
      const unsigned long long m = __ballot(bit);
      same &= bit ? m : ~m;
    }
    rank[r] = (uint32_t)__popcll(same & below);
    if (valid && rank[r] == 0) cnt[(r * WIRE_WAVES + wave) * WIRE_RADIX + d] = (uint32_t)__popcll(same);
  }
  __syncthreads();
  {
    const size_t e = (size_t)threadIdx.x * tiles + blockIdx.x;
    uint32_t run = hist[e] + sums[e / WIRE_SCAN_CHUNK];
#pragma unroll
    for (uint32_t k = 0; k < WIRE_ROUNDS * WIRE_WAVES; k++) {
      const uint32_t t = cnt[k * WIRE_RADIX + threadIdx.x];
      cnt[k * WIRE_RADIX + threadIdx.x] = run;
      run += t;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < WIRE_ROUNDS; r++) {
    const size_t j = base + (size_t)r * WIRE_BLOCK + threadIdx.x;
    if (j >= cells) continue;
    const size_t at = (size_t)cnt[(r * WIRE_WAVES + wave) * WIRE_RADIX + wire_digit(key[r], pass)] + rank[r];
    if (at >= cells) continue;                                  // cannot happen on counts that add up; never write outside the buffers
    k_out[at] = key[r];
    i_out[at] = i_in ? i_in[j] : (uint32_t)j;
  }
}

// one lane per position of the sorted order.  sig: S1 | S2 | S3, n values each (lag + 5n); roots: w^i, i < n.
__global__ void __launch_bounds__(WIRE_BLOCK) wire_link(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ idx, size_t cells,
                                                        const fr_t* __restrict__ roots, uint32_t log_n, fr_t* __restrict__ sig,
                                                        uint32_t* __restrict__ target) {
  const size_t j = (size_t)blockIdx.x * WIRE_BLOCK + threadIdx.x;
  if (j >= cells) return;
  const uint32_t cell = idx ? idx[j] : (uint32_t)j, pred = wire_pred(keys, idx, cells, j);
  if (cell >= cells || pred >= cells) return;                   // a permutation of the cells by construction
  const fr_t label = wire_label(load_fr(&roots[pred / 3]), pred % 3);
  store_fr(&sig[((size_t)(cell % 3) << log_n) + cell / 3], label);
  target[cell] = pred;
}

// one lane per row.  values: n_values Montgomery elements (slot 0 is never read: an empty wire is zero).  pi may be nullptr.
// status: the lowest cell whose id is not below n_values (the host sets ~0).
__global__ void __launch_bounds__(WIRE_BLOCK) wire_gather(const uint32_t* __restrict__ ids, size_t n, size_t n_public,
                                                          const fr_t* __restrict__ values, size_t n_values, fr_t* __restrict__ a,
                                                          fr_t* __restrict__ b, fr_t* __restrict__ c, fr_t* __restrict__ pi,
                                                          unsigned long long* __restrict__ status) {
  const size_t row = (size_t)blockIdx.x * WIRE_BLOCK + threadIdx.x;
  if (row >= n) return;
  fr_t left = Fr::zero();
#pragma unroll
  for (uint32_t col = 0; col < 3; col++) {
    const uint32_t id = ids[3 * row + col];
    fr_t v = Fr::zero();
    if (id != 0) {
      if (id < n_values) v = load_fr(&values[id]);
      else atomicMin(status, (unsigned long long)(3 * row + col));
    }
    if (col == 0) left = v;
    store_fr(&(col == 0 ? a : col == 1 ? b : c)[row], v);
  }
  if (pi) {
    fr_t p = Fr::zero();
    if (row < n_public) Fr::neg(p, left);
    store_fr(&pi[row], p);
  }
}

}  // namespace bp

// wire_plan.hpp -- everything bp_circuit_load_wires decides from numbers alone, and the same sort + link restated for the host.
// A circuit arrives as 3n variable ids (cell 3 * row + col, 0 = empty wire).  Program::make_s_polynomials (program.rs:76-147) groups
// the cells by id, row-major inside a group, and the NEXT cell of a group's cycle receives THIS cell's label (col + 1) w^row.  On the
// card that is a stable LSD radix sort of (id, cell) by id -- the payload starts as the identity, so stability alone keeps a group
// row-major -- and one link pass over the sorted order (wire_kernels.hpp).  This header holds the rules both sides share:
//   passes     8-bit digits, as many as the largest id needs: 0 (every id 0) .. 4
//   tiles      WIRE_TILE keys per workgroup and pass: a tile's 256 counts go to hist[digit * tiles + tile], so ONE exclusive scan of
//              hist is the first output position of (digit, tile) -- stable across tiles; inside a tile a key goes behind the keys of
//              its digit in front of it
//   scan       hist is scanned in chunks of WIRE_SCAN_CHUNK entries (one workgroup each) whose totals are scanned by one workgroup
//   link       position j of the sorted order holds cell idx[j]; its predecessor is idx[j - 1] inside a group and, for the head of a
//              group, the group's LAST cell, found by binary search for the upper bound of the key: S[cell] = label(pred), target[cell] = pred
// wire_sort_link_host runs exactly these steps with the functions below; tests/test_wire_plan.py holds it against bp_make_s_polynomials.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "host_codec.hpp"

namespace bp {

constexpr uint32_t WIRE_RADIX_BITS = 8, WIRE_RADIX = 1u << WIRE_RADIX_BITS;
constexpr uint32_t WIRE_BLOCK = 256;                                  // lanes per workgroup of every wire kernel: four waves of 64
constexpr uint32_t WIRE_WAVES = WIRE_BLOCK / 64;
constexpr uint32_t WIRE_ROUNDS = 8;                                   // keys per lane and tile
constexpr uint32_t WIRE_TILE = WIRE_BLOCK * WIRE_ROUNDS;              // keys per workgroup and pass
// wire_scatter ranks a tile in LDS: one count per (round, wave, digit), 32 KiB of the 64 a kernel has without asking for more
constexpr size_t WIRE_SCATTER_LDS = (size_t)WIRE_ROUNDS * WIRE_WAVES * WIRE_RADIX * sizeof(uint32_t);
constexpr uint32_t WIRE_SCAN_PER_LANE = 8;
constexpr uint32_t WIRE_SCAN_CHUNK = WIRE_BLOCK * WIRE_SCAN_PER_LANE; // hist entries per workgroup of wire_scan_chunks
constexpr uint32_t WIRE_SCAN_TILES = WIRE_SCAN_CHUNK / WIRE_RADIX;    // ... which is this many tiles' worth of one digit
constexpr uint32_t WIRE_MAX_LOG_N = 24;                               // bp_circuit_load's bound: 3 * 2^24 cells fit 32 bits

BP_HD uint32_t wire_passes(uint32_t max_id) {
  uint32_t p = 0;
  while (max_id) {
    p++;
    max_id >>= WIRE_RADIX_BITS;
  }
  return p;
}
BP_HD uint32_t wire_digit(uint32_t key, uint32_t pass) { return (key >> (WIRE_RADIX_BITS * pass)) & (WIRE_RADIX - 1); }
BP_HD uint32_t wire_ceil_div(size_t a, size_t b) { return (uint32_t)((a + b - 1) / b); }

// the launch shapes and buffer sizes of one load
struct WirePlan {
  uint32_t log_n;
  size_t cells;            // 3 * 2^log_n
  uint32_t passes;
  uint32_t tiles;          // grid of wire_hist and wire_scatter
  size_t hist_entries;     // WIRE_RADIX * tiles
  uint32_t scan_chunks;    // grid of wire_scan_chunks; one workgroup scans their totals
  uint32_t cell_blocks;    // grid of the one-lane-per-cell kernels (wire_max_id, wire_link)
  uint32_t row_blocks;     // grid of wire_gather (one lane per row)
  size_t key_bytes;        // ONE of the four sort buffers (keys and cells, in and out)
  size_t hist_bytes, sums_bytes;
  size_t sort_bytes;       // everything the sort holds while it runs
};
BP_HD WirePlan wire_plan(uint32_t log_n, uint32_t max_id) {
  WirePlan p;
  p.log_n = log_n;
  p.cells = (size_t)3 << log_n;
  p.passes = wire_passes(max_id);
  p.tiles = wire_ceil_div(p.cells, WIRE_TILE);
  p.hist_entries = (size_t)WIRE_RADIX * p.tiles;
  p.scan_chunks = wire_ceil_div(p.hist_entries, WIRE_SCAN_CHUNK);
  p.cell_blocks = wire_ceil_div(p.cells, WIRE_BLOCK);
  p.row_blocks = wire_ceil_div((size_t)1 << log_n, WIRE_BLOCK);
  p.key_bytes = p.cells * sizeof(uint32_t);
  p.hist_bytes = p.hist_entries * sizeof(uint32_t);
  p.sums_bytes = (size_t)p.scan_chunks * sizeof(uint32_t);
  p.sort_bytes = p.passes ? 4 * p.key_bytes + p.hist_bytes + p.sums_bytes : 0;
  return p;
}
// what the plan must satisfy for the kernels' 32-bit positions and the single-workgroup scan of the chunk totals
BP_HD bool wire_plan_valid(const WirePlan& p) {
  return p.log_n >= 3 && p.log_n <= WIRE_MAX_LOG_N && p.passes <= 4 && p.cells <= 0xffffffffu && (size_t)p.tiles * WIRE_TILE >= p.cells &&
         (size_t)(p.tiles - 1) * WIRE_TILE < p.cells && (size_t)p.scan_chunks * WIRE_SCAN_CHUNK >= p.hist_entries;
}

// the label of a cell from the table of roots: (col + 1) w^row, the factor by at most two additions
BP_HD fr_t wire_label(const fr_t& root, uint32_t col) {
  fr_t r = root;
  if (col >= 1) Fr::add(r, r, root);
  if (col >= 2) Fr::add(r, r, root);
  return r;
}
// first position in keys[0 .. cells) whose key is larger than `key` (the keys ascend)
BP_HD size_t wire_upper_bound(const uint32_t* keys, size_t cells, uint32_t key) {
  size_t lo = 0, hi = cells;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if (keys[mid] <= key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// the predecessor of the cell at position j of the sorted order; idx == nullptr: no pass ran, the order is the identity
BP_HD uint32_t wire_pred(const uint32_t* keys, const uint32_t* idx, size_t cells, size_t j) {
  const uint32_t key = keys[j];
  const size_t at = (j > 0 && keys[j - 1] == key) ? j - 1 : wire_upper_bound(keys, cells, key) - 1;
  return idx ? idx[at] : (uint32_t)at;
}

// ---- host restatement: the passes, tile by tile and chunk by chunk as the kernels take them, then the link.  s1 s2 s3: 2^log_n
// Montgomery values each; target: 3 * 2^log_n cells (target[cell] = the cell whose label S holds at `cell`).  *passes_out: passes run.
inline void wire_sort_link_host(uint32_t log_n, const uint32_t* wire_ids, fr_t* s1, fr_t* s2, fr_t* s3, uint32_t* target, uint32_t* passes_out) {
  uint32_t max_id = 0;
  for (size_t k = 0; k < ((size_t)3 << log_n); k++) max_id = wire_ids[k] > max_id ? wire_ids[k] : max_id;
  const WirePlan p = wire_plan(log_n, max_id);
  const size_t cells = p.cells, n = (size_t)1 << log_n;
  std::vector<uint32_t> keys[2], idx[2], hist(p.hist_entries), sums(p.scan_chunks);
  const uint32_t* k_in = wire_ids;
  const uint32_t* i_in = nullptr;
  for (uint32_t pass = 0; pass < p.passes; pass++) {
    std::vector<uint32_t>&k_out = keys[pass & 1], &i_out = idx[pass & 1];
    k_out.resize(cells);
    i_out.resize(cells);
    for (uint32_t t = 0; t < p.tiles; t++) {                                   // wire_hist
      for (uint32_t d = 0; d < WIRE_RADIX; d++) hist[(size_t)d * p.tiles + t] = 0;
      for (size_t j = (size_t)t * WIRE_TILE; j < cells && j < (size_t)(t + 1) * WIRE_TILE; j++) hist[(size_t)wire_digit(k_in[j], pass) * p.tiles + t]++;
    }
    for (uint32_t c = 0; c < p.scan_chunks; c++) {                             // wire_scan_chunks: exclusive inside a chunk, the total aside
      uint32_t run = 0;
      for (size_t e = (size_t)c * WIRE_SCAN_CHUNK; e < p.hist_entries && e < (size_t)(c + 1) * WIRE_SCAN_CHUNK; e++) {
        const uint32_t v = hist[e];
        hist[e] = run;
        run += v;
      }
      sums[c] = run;
    }
    uint32_t run = 0;                                                          // wire_scan_sums
    for (uint32_t c = 0; c < p.scan_chunks; c++) {
      const uint32_t v = sums[c];
      sums[c] = run;
      run += v;
    }
    for (uint32_t t = 0; t < p.tiles; t++) {                                   // wire_scatter
      uint32_t seen[WIRE_RADIX] = {0};
      for (size_t j = (size_t)t * WIRE_TILE; j < cells && j < (size_t)(t + 1) * WIRE_TILE; j++) {
        const uint32_t d = wire_digit(k_in[j], pass);
        const size_t e = (size_t)d * p.tiles + t;
        const size_t at = (size_t)hist[e] + sums[e / WIRE_SCAN_CHUNK] + seen[d]++;
        k_out[at] = k_in[j];
        i_out[at] = i_in ? i_in[j] : (uint32_t)j;
      }
    }
    k_in = k_out.data();
    i_in = i_out.data();
  }
  fr_t w;
  host_root_of_unity(w, n);
  std::vector<fr_t> root(n);
  root[0] = Fr::one();
  for (size_t i = 1; i < n; i++) Fr::mul(root[i], root[i - 1], w);
  fr_t* out[3] = {s1, s2, s3};
  for (size_t j = 0; j < cells; j++) {                                         // wire_link
    const uint32_t cell = i_in ? i_in[j] : (uint32_t)j, pred = wire_pred(k_in, i_in, cells, j);
    out[cell % 3][cell / 3] = wire_label(root[pred / 3], pred % 3);
    target[cell] = pred;
  }
  if (passes_out) *passes_out = p.passes;
}

}  // namespace bp

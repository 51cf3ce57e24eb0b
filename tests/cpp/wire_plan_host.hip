// wire_plan_host.hip -- TEST-ONLY host build of csrc/wire_plan.hpp: the pass count, digit, tile and grid rules of bp_circuit_load_wires
// and the host restatement of its sort + link, so tests/test_wire_plan.py checks on the CPU the rules the kernels of wire_kernels.hpp
// run by.  Built by that test into its tmp_path; never linked into the product library.
#include "../../baby_plonk_rust_amd/csrc/wire_plan.hpp"
using namespace bp;

extern "C" {
// tile | scan chunk | tiles per scan chunk | lanes per workgroup | radix | LDS bytes of the scatter
void wp_consts(uint64_t out[6]) {
  out[0] = WIRE_TILE;
  out[1] = WIRE_SCAN_CHUNK;
  out[2] = WIRE_SCAN_TILES;
  out[3] = WIRE_BLOCK;
  out[4] = WIRE_RADIX;
  out[5] = WIRE_SCATTER_LDS;
}
uint32_t wp_passes(uint32_t max_id) { return wire_passes(max_id); }
uint32_t wp_digit(uint32_t key, uint32_t pass) { return wire_digit(key, pass); }
// cells | passes | tiles | hist_entries | scan_chunks | cell_blocks | row_blocks | key_bytes | hist_bytes | sums_bytes | sort_bytes; returns valid
int wp_plan(uint32_t log_n, uint32_t max_id, uint64_t out[11]) {
  const WirePlan p = wire_plan(log_n, max_id);
  const uint64_t v[11] = {p.cells, p.passes, p.tiles, p.hist_entries, p.scan_chunks, p.cell_blocks, p.row_blocks, p.key_bytes, p.hist_bytes, p.sums_bytes, p.sort_bytes};
  for (int i = 0; i < 11; i++) out[i] = v[i];
  return wire_plan_valid(p) ? 1 : 0;
}
// the host restatement: s1 s2 s3 (2^log_n x 32 bytes, Montgomery), target (3 * 2^log_n words); returns the passes it ran
uint32_t wp_sort_link(uint32_t log_n, const uint32_t* wire_ids, void* s1, void* s2, void* s3, uint32_t* target) {
  uint32_t passes = 0;
  wire_sort_link_host(log_n, wire_ids, (fr_t*)s1, (fr_t*)s2, (fr_t*)s3, target, &passes);
  return passes;
}
}

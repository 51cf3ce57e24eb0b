// msm_plan_host.hip -- TEST-ONLY host build of csrc/msm_plan.hpp (limits, knobs and plan of the G1 MSM pipeline).  Built by
// tests/test_msm_plan.py into its tmp_path; never linked into the product library.  With -DMSM_PLAN_MAIN it is a stand-alone program
// (its own main: the sweep of the test, every plan once) for a sanitizer run on the CPU (not a pytest test, never run on a GPU):
//   hipcc --offload-host-only -O1 -g -DMSM_PLAN_MAIN -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/cpp/msm_plan_host.hip -o msm_plan_main && ./msm_plan_main
#include "../../baby_plonk_rust_amd/csrc/msm_plan.hpp"
using namespace bp;

// The fourteen BP_MSM_* variables as words, in the order of KNOB_NAMES; MP_UNSET = the variable is absent.  The rule of knob_u32 (ctx.hpp)
// restated: a value outside [lo, hi] leaves the default.
constexpr uint32_t MP_UNSET = 0xffffffffu;
static const char* const KNOB_NAMES[14] = {"BP_MSM_C", "BP_MSM_CHUNK", "BP_MSM_RADIX", "BP_MSM_RADIX_FROM", "BP_MSM_RADIX_BITS", "BP_MSM_PACKED", "BP_MSM_SORT",
                                           "BP_MSM_PART_SLICE", "BP_MSM_PART_WIDE8", "BP_MSM_COUNT_SLICE", "BP_MSM_PART_FLAT", "BP_MSM_FINAL_THREADS",
                                           "BP_MSM_FIXUP", "BP_MSM_PLANES_WIDE_MIN"};
static MsmKnobs knobs_of(const uint32_t* env) {
  return msm_knobs_read([env](const char* name, uint32_t dflt, uint32_t lo, uint32_t hi) {
    for (int i = 0; i < 14; i++)
      if (!strcmp(name, KNOB_NAMES[i])) return env[i] == MP_UNSET || env[i] < lo || env[i] > hi ? dflt : env[i];
    return dflt;
  });
}

constexpr int MP_WORDS = 64, MP_STEP_WORDS = 8;
extern "C" {
// the plan of msm_plan(J, n_each, table_c, table_stride, blob, knobs read from env).  Returns the refusal's code (0: none) and its text in
// `what`.  out (MP_WORDS x u64), in this order:
//   0 empty, 1 valid (msm_plan_valid), 2 entries, 3 n_chunks, 4 kb, 5 pb, 6 rbits, 7 vb, 8 sort, 9 packed, 10 flat, 11 wide8,
//   12..21 level 1: pb, rb, slice, n_slices, slice1, n_slices1, count_threads, scatter_threads, cap, part_lds,
//   22 lv0, 23 lv1, 24 gx2, 25 n_sub, 26 shift2, 27 scan_tiles, 28 n_final, 29 final_grid, 30 final_threads, 31 long_gx, 32 long_gy, 33 rhist,
//   34 long_cap, 35 ctl_words, 36 ctl_zeroed, 37 run_ticket, 38 acc_grid, 39 by_edges, 40 fixup_grid, 41 quads, 42 per_window, 43 n_planes, 44 Wr,
//   45 n_wide, 46 n_steps, 47 tmp_slots0, 48 tmp_slots1
// dev: the MsmPlan as 33 words; steps: n_steps x (kind, out, k, m, nodes, gx, gy, lds); ws: the 22 workspace sizes in MsmWsBytes' order;
// path: the words of bp_msm_last_path
int mp_plan(uint32_t J, const uint64_t* n_each, uint32_t table_c, uint64_t table_stride, int blob, const uint32_t* env, uint64_t* out, uint32_t* dev,
            uint32_t* steps, uint64_t* ws, uint32_t* path, char* what) {
  size_t n[MSM_MAX_BATCH + 4] = {0};
  for (uint32_t j = 0; j < J && j < MSM_MAX_BATCH + 4; j++) n[j] = (size_t)n_each[j];
  const MsmHostPlan hp = msm_plan(J, n, table_c, (size_t)table_stride, blob != 0, knobs_of(env));
  what[0] = 0;
  if (hp.what) strncpy(what, hp.what, 63), what[63] = 0;
  const MsmLevel1& s = hp.l1;
  const uint64_t w[] = {hp.empty, (uint64_t)(!hp.err && !hp.empty && msm_plan_valid(hp)), hp.entries, hp.n_chunks, hp.kb, hp.pb, hp.rbits, hp.vb, hp.sort, hp.packed,
                        hp.flat, hp.wide8, s.pb, s.rb, s.slice, s.n_slices, s.slice1, s.n_slices1, s.count_threads, s.scatter_threads, s.cap, s.part_lds, hp.lv[0],
                        hp.lv[1], hp.gx2, hp.n_sub, hp.shift2, hp.scan_tiles, hp.n_final, hp.final_grid, hp.final_threads, hp.long_gx, hp.long_gy, hp.rhist,
                        hp.long_cap, hp.ctl_words, hp.ctl_zeroed, hp.run_ticket, hp.acc_grid, hp.by_edges, hp.fixup_grid, hp.quads, hp.per_window, hp.n_planes,
                        hp.Wr, hp.n_wide, hp.n_steps, hp.tmp_slots[0], hp.tmp_slots[1]};
  static_assert(sizeof w / sizeof w[0] <= MP_WORDS, "out");
  for (int i = 0; i < MP_WORDS; i++) out[i] = i < (int)(sizeof w / sizeof w[0]) ? w[i] : 0;
  static_assert(sizeof(MsmPlan) == 33 * 4, "MsmPlan travels to the kernels: its layout is fixed");
  memcpy(dev, &hp.dev, sizeof hp.dev);
  for (uint32_t i = 0; i < hp.n_steps; i++) {
    const MsmTreeStep& t = hp.step[i];
    const uint32_t f[MP_STEP_WORDS] = {t.kind, t.out, t.k, t.m, t.nodes, t.gx, t.gy, t.lds};
    memcpy(steps + MP_STEP_WORDS * i, f, sizeof f);
  }
  static_assert(sizeof(MsmWsBytes) == 22 * sizeof(size_t), "22 workspaces");
  for (int i = 0; i < 22; i++) ws[i] = ((const size_t*)&hp.ws)[i];
  if (!hp.err && !hp.empty) msm_plan_path(hp, path);
  return hp.err;
}
void mp_default_knobs(uint32_t* w) {
  const MsmKnobs kn;
  const uint32_t f[14] = {kn.c, kn.chunk, kn.radix, kn.radix_from, kn.radix_bits, kn.packed, kn.sort, kn.part_slice, kn.part_wide8, kn.count_slice, kn.part_flat,
                          kn.final_threads, kn.fixup, kn.planes_wide_min};
  memcpy(w, f, sizeof f);
}
uint32_t mp_windows(uint32_t c) { return msm_windows(c); }
// R, m[8], bias[9] of msm_table_radix(c, knobs): all zero when the width keeps power-of-two windows
void mp_table_radix(uint32_t c, const uint32_t* env, uint32_t* out) {
  const MsmRadix* rx = msm_table_radix(c, knobs_of(env));
  memset(out, 0, 18 * 4);
  if (rx) out[0] = rx->R, memcpy(out + 1, rx->m, 32), memcpy(out + 9, rx->bias, 36);
}
uint32_t mp_auto_width(uint64_t n) { return srs_auto_width(n); }
int mp_width_pays(uint32_t c, uint64_t n) { return srs_width_pays(c, (size_t)n); }
void mp_limits(uint64_t* out) {
  const uint64_t f[18] = {MSM_MAX_C, MSM_MAX_TABLE_C, MSM_HIST_LOG, MSM_MAX_WINDOWS, MSM_MAX_BATCH, SCAN_TILE, RADIX_SLICE, PART_MAX_BITS, PART_MAX, FIXUP_LONG,
                          FIXUP_LONG_SLICES, FIXUP_LONG_SPLIT_FROM, PLANES_STEP_LOG, MSM_SLOT_BYTES, MSM_LDS_RADIX_SCATTER, MSM_LDS_RUN_HIST, MSM_LDS_PART_SCATTER,
                          MSM_LDS_DEFAULT};
  memcpy(out, f, sizeof f);
}
}

#ifdef MSM_PLAN_MAIN
#include <stdio.h>
// the sweep of tests/test_msm_plan.py: every n, width and batch under the default knobs and under each knob alone at both ends of its range
// and one value outside it; every plan that is not refused must pass msm_plan_valid
int main() {
  static const uint32_t ends[14][3] = {{2, 16, 17},  {1, 1024, 1025}, {0, 1, 2},        {8, 30, 7},  {0, 16, 17},       {0, 2, 3},   {1, 2, 0},
                                       {64, 4096, 63}, {0, 1, 2},     {64, 65536, 63}, {0, 2, 3},   {256, 1024, 255}, {0, 2, 3},   {256, 1u << 30, 255}};
  uint64_t sizes[80], out[MP_WORDS], ws[22];
  uint32_t dev[33], steps[MP_STEP_WORDS * MSM_MAX_TREE_STEPS], path[12], n_sizes = 0;
  char what[64];
  for (uint64_t n : {1ull, 2ull, 31ull, 32ull, 33ull, (1ull << 20) + 6, (1ull << 31) - 1, 1ull << 31, 0ull}) sizes[n_sizes++] = n;
  for (uint32_t k = 5; k <= 24; k++)
    for (int d = -1; d <= 1; d++) sizes[n_sizes++] = (1ull << k) + d;
  unsigned long plans = 0, refused = 0;
  for (int knob = -1; knob < 14; knob++)
    for (int v = 0; v < (knob < 0 ? 1 : 3); v++) {
      uint32_t env[14];
      for (int i = 0; i < 14; i++) env[i] = i == knob ? ends[i][v] : MP_UNSET;
      for (uint32_t si = 0; si < n_sizes; si++)
        for (uint32_t tc = 0; tc <= 25; tc++) {
          if (tc >= 1 && tc <= 3) continue;
          for (uint32_t J = 0; J <= 5; J++)
            for (int blob = 0; blob < 2; blob++) {
              const uint64_t n = sizes[si], n_each[8] = {J > 1 ? n / 2 + 1 : n, n, n / 3, 1, 0, 0, 0, 0};
              const int err = mp_plan(J, n_each, tc, n, blob, env, out, dev, steps, ws, path, what);
              if (err) { refused++; continue; }
              plans++;
              if (!out[0] && !out[1]) { printf("invalid plan: knob %d value %u n %llu table_c %u J %u\n", knob, knob < 0 ? 0 : ends[knob][v], (unsigned long long)n, tc, J); return 1; }
            }
        }
    }
  uint32_t rx[18];
  uint32_t env[14];
  for (int i = 0; i < 14; i++) env[i] = MP_UNSET;
  for (uint32_t c = 2; c <= 24; c++) mp_table_radix(c, env, rx), plans += mp_windows(c) + rx[0] % 2;
  printf("msm_plan_host ok (%lu plans, %lu refusals)\n", plans, refused);
  return 0;
}
#endif

// ntt_plan_host.hip -- TEST-ONLY host build of csrc/ntt_plan.hpp (tile layout, kernel limits, knobs and plan of the Fr NTT).  Built by
// tests/test_ntt_plan.py into its tmp_path; never linked into the product library.  With -DNTT_PLAN_MAIN it is a stand-alone program
// (its own main: every plan and every layout once) for a sanitizer run on the CPU (not a pytest test, never run on a GPU):
//   hipcc --offload-host-only -O1 -g -DNTT_PLAN_MAIN -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/cpp/ntt_plan_host.hip -o ntt_plan_main && ./ntt_plan_main
#include "../../baby_plonk_rust_amd/csrc/ntt_plan.hpp"
using namespace bp;

// knobs as eleven words: three_pass_from, cols_log[4], split_k, split_l[3], swizzle, lanes_shift (0xffffffff in cols_log: no override)
static NttKnobs knobs_of(const uint32_t* w) {
  NttKnobs kn;
  kn.three_pass_from = w[0];
  for (int i = 0; i < 4; i++) kn.cols_log[i] = w[1 + i];
  kn.split_k = w[5];
  for (int i = 0; i < 3; i++) kn.split_l[i] = w[6 + i];
  kn.swizzle = w[9];
  kn.lanes_shift = w[10];
  return kn;
}
extern "C" {
void np_default_knobs(uint32_t* w, uint32_t* full_twiddles_max_log, uint32_t* group_split_from) {
  const NttKnobs kn;
  w[0] = kn.three_pass_from;
  for (int i = 0; i < 4; i++) w[1 + i] = kn.cols_log[i];
  w[5] = kn.split_k;
  for (int i = 0; i < 3; i++) w[6 + i] = kn.split_l[i];
  w[9] = kn.swizzle;
  w[10] = kn.lanes_shift;
  *full_twiddles_max_log = kn.full_twiddles_max_log;
  *group_split_from = kn.group_split_from;
}
// out: k, P, h, then l, s, cl, swizzled, threads, lds_bytes, tiles of each of three passes; dev: the NttPlan that travels to the kernel
// (k, P, l[4], cl[4], h); returns ntt_plan_valid of what ntt_plan gave
int np_plan(uint32_t k, const uint32_t* knobs, uint32_t* out, uint32_t* dev) {
  const NttHostPlan p = ntt_plan(k, knobs_of(knobs));
  out[0] = p.dev.k; out[1] = p.dev.P; out[2] = p.dev.h;
  for (int i = 0; i < 3; i++) {
    const NttPass& q = p.pass[i];
    const uint32_t f[7] = {q.l, q.s, q.cl, q.swizzled, q.threads, q.lds_bytes, q.tiles};
    for (int j = 0; j < 7; j++) out[3 + 7 * i + j] = i < (int)p.dev.P ? f[j] : 0;
  }
  static_assert(sizeof(NttPlan) == 11 * 4, "eleven words");
  for (int i = 0; i < 11; i++) dev[i] = ((const uint32_t*)&p.dev)[i];
  return ntt_plan_valid(p);
}
int np_full_tables(uint32_t k, uint32_t max_log) {
  NttKnobs kn;
  kn.full_twiddles_max_log = max_log;
  return ntt_plan(k, kn).full_tables;
}
int np_split_ok(uint32_t k, const uint32_t* knobs, uint32_t parts) { return ntt_split_ok(ntt_plan(k, knobs_of(knobs)), parts); }
void np_tile(uint32_t l, uint32_t cl, int swizzled, uint32_t* out) {
  const NttTile t = ntt_tile(l, cl, swizzled != 0);
  out[0] = t.CP; out[1] = t.tstride; out[2] = t.tw_off; out[3] = t.tw_slots; out[4] = t.lds_bytes;
}
int np_tile_swizzled(uint32_t l, uint32_t cl, int on) { return ntt_tile_swizzled(l, cl, on != 0); }
uint32_t np_tile_at(int swizzled, uint32_t row, uint32_t c, uint32_t CP) { return swizzled ? tile_at<true>(row, c, CP) : tile_at<false>(row, c, CP); }
void np_limits(uint32_t* out) {
  out[0] = NTT_PAD_THREADS; out[1] = NTT_PAD_LDS_MAX; out[2] = NTT_SWZ_THREADS; out[3] = NTT_SWZ_LDS_MAX; out[4] = NTT_SMALL_THREADS;
  out[5] = NTT_MAX_PASS_LOG; out[6] = NTT_SMALL_MAX_LOG;
}
}

#ifdef NTT_PLAN_MAIN
#include <stdio.h>
int main() {
  unsigned long sum = 0;
  uint32_t w[11], a, b, out[24], dev[11];
  np_default_knobs(w, &a, &b);
  for (uint32_t k = 0; k <= 40; k++)
    for (uint32_t tpf = 11; tpf <= 29; tpf++)
      for (uint32_t c = 0; c < 5; c++)
        for (uint32_t sp = 0; sp < 11 * 11 * 11; sp++) {
          uint32_t v[11] = {tpf, c < 4 ? c : w[1], c < 4 ? c : w[2], c < 4 ? c : w[3], c < 4 ? c : w[4], k, sp / 121, sp / 11 % 11, sp % 11, c & 1, c >> 1 & 1};
          if (sp && tpf != 20) continue;
          if (!np_plan(k, v, out, dev) && k <= 28) { printf("invalid plan: k %u tpf %u c %u split %u\n", k, tpf, c, sp); return 1; }
          sum += out[1] + np_split_ok(k, v, 1u << (sp % 4));
        }
  for (uint32_t l = 0; l <= 10; l++)
    for (uint32_t cl = 0; cl <= 3; cl++)
      for (int swz = 0; swz < 2; swz++) {
        np_tile(l, cl, swz, out);
        for (uint32_t row = 0; row < (1u << l); row++) sum += np_tile_at(swz && np_tile_swizzled(l, cl, 1), row, (1u << cl) - 1, out[0]);
      }
  printf("ntt_plan_host ok (%lu)\n", sum);
  return 0;
}
#endif

// ntt_plan.hpp -- everything the Fr NTT decides from numbers alone: the LDS tile layout (one definition, used by the kernels of
// ntt_kernels.hpp for their addresses and by the host for the bytes it asks for), the kernels' limits, the experiment knobs and the
// plan of a transform (passes, digit widths, tile shapes, launch shapes), validated as a whole.  The host part is pure: no HIP
// runtime call and no bp_ctx; tests/test_ntt_plan.py compiles it for the host alone and enumerates it.
#pragma once
#include <stdint.h>

#include "bigint.hpp"      // BP_HD

namespace bp {

constexpr int NTT_MAX_PASS_LOG = 10;    // per-pass transform length up to 2^10
constexpr int NTT_SMALL_MAX_LOG = 10;   // single-workgroup transform up to 2^10
constexpr uint32_t NTT_LIMBS = 9;       // an element in LDS: 9 x 29-bit limbs, 36 bytes (fr29.hpp N29; ntt_kernels.hpp asserts the match)

// ---- kernel limits: __launch_bounds__, the hipFuncSetAttribute calls of ntt_init_tables and the plan's checks all read these
// padded tiles (ntt_pass_strided, ntt_pass_last) and ntt_small: a radix-4 group needs ~140 registers, so 512 lanes at most
constexpr uint32_t NTT_PAD_THREADS = 512, NTT_PAD_LDS_MAX = 160 * 1024;
// swizzled tiles (ntt_pass_*_swz): 2^l x 8 tiles, l <= 7, 256 lanes, three workgroups per CU
constexpr uint32_t NTT_SWZ_THREADS = 256, NTT_SWZ_LDS_MAX = 64 * 1024, NTT_SWZ_PER_CU = 3;
constexpr uint32_t NTT_SMALL_THREADS = 256;
constexpr uint32_t ntt_threads_max(bool swizzled) { return swizzled ? NTT_SWZ_THREADS : NTT_PAD_THREADS; }
constexpr uint32_t ntt_lds_max(bool swizzled) { return swizzled ? NTT_SWZ_LDS_MAX : NTT_PAD_LDS_MAX; }

// tile columns C = 2^cl shrink as the per-pass length grows so that TWO tiles (2^l x (C+1) x 36 B each, plus stage twiddles)
// fit the 160 KiB of LDS wherever possible: with one 1 024-lane workgroup per CU nothing overlaps a tile's global loads and
// stores, with two the other one computes meanwhile (measured, profiles/r02_ntt_tile_width_ab.txt: l = 8: C = 8 -> 4 is -8 %
// at 2^22 and 2^24; l = 9: C = 4 -> 2 is -25 % at 2^18).  l <= 7 -> C = 8 (256-B global runs), l = 8 -> 4, l = 9 -> 2,
// l = 10 -> 2 (one tile per CU: a single column would halve the run to 32 B and measured +32 %)
BP_HD constexpr uint32_t ntt_tile_cols_log(uint32_t l) { return l <= 7 ? 3u : (l == 8 ? 2u : 1u); }
BP_HD constexpr uint32_t ntt_tw_slots(uint32_t l) { return (1u << l) < 4 ? 2u : (1u << l) >> 1; }

// Tile addressing, element (row, c) of a tile of 2^l rows x C columns:
//   padded   (SWZ = false): row * CP + c with CP = C + 1 (a single column needs no pad);
//   swizzled (SWZ = true, C = 8 and l <= 7 only): no pad -- ((row ^ z(row)) << 3) | c, where z puts the parity of row bits
//            2, 4, 6 into bit 0 and the parity of bits 3, 5 into bit 1.  Every access pattern of a pass (the fill: consecutive
//            rows; a stage: rows j, j + 1, .. of one block, or -- last stage pairs -- rows 4 or 8 apart; the drain: rows in
//            bit-reversed order, i.e. 64, 32, 96 apart) then spreads the 8-element groups of the lanes of one LDS cycle over
//            different banks, which the one-element pad does not do for the drain (row pitch 72 B: rows 16 apart collide).
//            Without the pad a 2^7 x 8 tile plus its stage twiddles is 39 KiB (four would fit a CU; the butterflies' 129 registers
//            allow three workgroups = three waves per SIMD, and tools/ntt_occupancy_probe.sh shows the pass time does not depend on
//            the residency: T = 10 us + 11 us per tile per CU with one, three or four resident -- the VALU is the bound).
BP_HD uint32_t ntt_popc(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(x);
#else
  return (uint32_t)__builtin_popcount(x);
#endif
}
template <bool SWZ>
BP_HD uint32_t tile_at(uint32_t row, uint32_t c, uint32_t CP) {
  if (SWZ) {
    const uint32_t z = (ntt_popc(row & 0x54u) & 1u) | ((ntt_popc(row & 0x28u) & 1u) << 1);
    return ((row ^ z) << 3) | c;
  }
  return row * CP + c;
}
// 2^l x 8 tiles with 2 <= l <= 7 run unpadded with swizzled rows (39 KiB at l = 7, bank-conflict-free drain); BP_NTT_SWIZZLE=0: padded
BP_HD constexpr bool ntt_tile_swizzled(uint32_t l, uint32_t cl, bool swizzle_on) { return swizzle_on && cl == 3 && l <= 7 && l >= 2; }

// THE layout of a tile of 2^l rows x 2^cl columns in dynamic LDS: the elements limb-major with element stride `tstride` (even: the
// limb-pair arrays stay 8-byte aligned); behind them the stage twiddles, ntt_tw_slots(l) elements with that count as their stride;
// 16 bytes of slack.  ntt_small's single tile is the one-column form, ntt_tile(k, 0, false).
// The three rules are functions of their own, in rows L = 2^l and columns C = 2^cl: a kernel applies them to the L, C and L * CP it
// holds anyway (CP = SWZ ? C : ntt_tile_pitch(C)) -- handed l and cl, the compiler shifts and keeps registers differently and the
// kernels' code changes.  ntt_tile puts the same three together for the host.
// row pitch of a padded tile in elements (a single column needs no pad); a swizzled tile has none: its pitch is C (tile_at)
BP_HD constexpr uint32_t ntt_tile_pitch(uint32_t C) { return C == 1 ? C : C + 1; }
BP_HD constexpr uint32_t ntt_tile_stride(uint32_t cells) { return (cells + 1) & ~1u; }      // cells = rows x pitch; elements per limb plane
BP_HD constexpr uint32_t ntt_tile_tw_off(uint32_t tstride) { return NTT_LIMBS * tstride; }      // first dword of the twiddle area
struct NttTile {
  uint32_t CP, tstride, tw_off, tw_slots;
  uint32_t lds_bytes;    // dynamic LDS of the launch
};
BP_HD constexpr NttTile ntt_tile(uint32_t l, uint32_t cl, bool swizzled) {
  const uint32_t C = 1u << cl, CP = swizzled ? C : ntt_tile_pitch(C), tstride = ntt_tile_stride((1u << l) * CP), slots = ntt_tw_slots(l);
  return {CP, tstride, ntt_tile_tw_off(tstride), slots, (tstride + slots) * NTT_LIMBS * 4 + 16};
}

// ---- the experiment knobs (BP_NTT_*, docs/EXPERIMENTS.md).  The initialisers are the shipped behaviour; ntt.hip's ntt_knobs() fills
// the struct from the environment in the experiment build, on every call.
constexpr uint32_t NTT_COLS_AUTO = 0xffffffffu;
struct NttKnobs {
  // 2^20 as 7 + 7 + 6: small tiles keep three workgroups per CU busy (0.152 ms against 0.159 for 10 + 10, whose 74-KiB tiles
  // leave one 512-lane workgroup per CU); 2^19 stays 10 + 9 (0.080 against 0.084).  profiles/r02_ntt_radix4_ab.txt
  uint32_t three_pass_from = 20;                                                       // BP_NTT_THREE_PASS_FROM, 11..29
  // BP_NTT_COLS_LOG_L7 (every l <= 7), _L8, _L9, _L10, 0..3: cl of the passes of that width; AUTO = ntt_tile_cols_log above
  uint32_t cols_log[4] = {NTT_COLS_AUTO, NTT_COLS_AUTO, NTT_COLS_AUTO, NTT_COLS_AUTO};
  // BP_NTT_SPLIT="k:l1,l2,l3" replaces the digit widths of one size (l3 = 0: two passes); split_k = 0: none
  uint32_t split_k = 0, split_l[3] = {0, 0, 0};
  uint32_t swizzle = 1;                                                                // BP_NTT_SWIZZLE, 0 / 1: see ntt_tile_swizzled
  // BP_NTT_LANES_SHIFT = 1 doubles the lanes of a pass (they only help the load / store phases), up to the kernel's bound
  uint32_t lanes_shift = 0;
  // the inter-pass twiddles as full tables for N <= 2^24 (48 B per entry: 50 MB at 2^20, 805 MB at 2^24); above, the two-level lookup
  uint32_t full_twiddles_max_log = 24;                                                 // BP_NTT_FULL_TWIDDLES_MAX_LOG, 0..28
  uint32_t group_split_from = 22;      // BP_NTT_GROUP_SPLIT_FROM, 11..29: a group context cuts one host transform over its members from here
};

// ---- the plan
struct NttPlan {         // what travels to the last pass in the kernarg segment (NttLastArgs): the kernels depend on these bytes
  uint32_t k;            // log2 N
  uint32_t P;            // passes
  uint32_t l[4];         // digit widths
  uint32_t cl[4];        // log2 of the tile's column count per pass (ntt_tile_cols_log unless overridden)
  uint32_t h;            // low table has 2^h entries, high table 2^(k-h)
};
static_assert(sizeof(NttPlan) == 44, "NttPlan is part of the kernarg segment of ntt_pass_last");
struct NttPass {
  uint32_t l, s, cl;     // digit width, bits below the digit (0 for the last pass), log2 of the tile's columns
  bool swizzled;         // which kernel: ntt_pass_*_swz or the padded one
  uint32_t threads, lds_bytes, tiles;        // block, dynamic LDS and grid.x of the whole pass
};
struct NttHostPlan {
  NttPlan dev;
  NttPass pass[3];
  bool full_tables;      // the strided passes multiply by full inter-pass twiddle tables (built on first use) instead of the two-level lookup
};

// one radix-4 group (four elements, two stages in registers) per lane: 2^(l-2) * columns lanes, at least a wave, at most the chosen
// kernel's launch bound
inline NttPass ntt_pass(uint32_t k, uint32_t l, uint32_t s, uint32_t cl, const NttKnobs& kn) {
  NttPass p = {l, s, cl, ntt_tile_swizzled(l, cl, kn.swizzle != 0), 0, 0, 0};
  const uint32_t t = (((1u << l) << cl) >> 2) << kn.lanes_shift, cap = ntt_threads_max(p.swizzled);
  p.threads = t > cap ? cap : (t < 64 ? 64 : t);
  p.lds_bytes = ntt_tile(l, cl, p.swizzled).lds_bytes;
  p.tiles = l + cl <= k ? 1u << (k - l - cl) : 0;
  return p;
}
// ntt_small: the whole transform is one single-column tile, one workgroup
inline NttPass ntt_small_pass(uint32_t k) { return {k, 0, 0, false, NTT_SMALL_THREADS, ntt_tile(k, 0, false).lds_bytes, 1}; }
inline bool ntt_pass_fits(const NttPass& p, uint32_t threads_max) { return p.lds_bytes <= ntt_lds_max(p.swizzled) && p.threads <= threads_max; }
inline uint32_t ntt_cols_log(uint32_t k, uint32_t l, const NttKnobs& kn) {
  const uint32_t over = kn.cols_log[l <= 7 ? 0 : l - 7];
  if (over == NTT_COLS_AUTO) return ntt_tile_cols_log(l);
  const NttPass p = ntt_pass(k, l, 0, over > 3 ? 3 : over, kn);
  return ntt_pass_fits(p, ntt_threads_max(p.swizzled)) ? p.cl : ntt_tile_cols_log(l);      // an override must still fit the LDS
}

// the widths sum to k, each <= 10; every tile has whole columns (strided: s >= cl) or whole rows e_1 (last: l_1 >= cl); LDS and
// threads within the chosen kernel's limits
inline bool ntt_plan_valid(const NttHostPlan& p) {
  const uint32_t P = p.dev.P;
  uint32_t sum = 0;
  if (P < 1 || P > 3 || (P == 1) != (p.dev.k <= (uint32_t)NTT_SMALL_MAX_LOG)) return false;
  for (uint32_t i = 0; i < P; i++) {
    const NttPass& q = p.pass[i];
    sum += q.l;
    if (q.l > (uint32_t)NTT_MAX_PASS_LOG || !ntt_pass_fits(q, P == 1 ? NTT_SMALL_THREADS : ntt_threads_max(q.swizzled)) || q.tiles == 0) return false;
    if (i + 1 < P ? q.s < q.cl : p.pass[0].l < q.cl) return false;
  }
  return sum == p.dev.k;
}

// the plan the knobs ask for, valid or not
inline NttHostPlan ntt_plan_unchecked(uint32_t k, const NttKnobs& kn) {
  uint32_t P = k <= (uint32_t)NTT_SMALL_MAX_LOG ? 1 : (k <= 2 * (uint32_t)NTT_MAX_PASS_LOG ? 2 : 3), l[3] = {0, 0, 0}, cl[3] = {0, 0, 0};
  if (P == 2 && k >= kn.three_pass_from) P = 3;
  uint32_t rem = k;
  for (uint32_t i = 0; i < P; i++) {          // balanced widths, larger ones first
    l[i] = (rem + P - i - 1) / (P - i);
    rem -= l[i];
    cl[i] = P == 1 ? 0 : ntt_cols_log(k, l[i], kn);
  }
  // three passes of widths (a, a, a - 1) with 8-column tiles everywhere (a <= 7: 2^20 = 7 + 7 + 6): the short digit goes in the MIDDLE --
  // the last pass pays no inter-pass twiddle product, so it is the cheapest place for a stage: 0.148 against 0.152 ms at 2^20, three alternating
  // rounds (profiles/r05_ntt_order_ab.txt); 2^22 (8, 7, 7) and 2^23 (8, 8, 7) show no difference between the orders and keep theirs
  if (P == 3 && l[0] <= 7 && l[0] == l[1] && l[2] + 1 == l[1]) {
    l[1] = l[2];
    l[2] = l[0];
    for (uint32_t i = 1; i < 3; i++) cl[i] = ntt_tile_cols_log(l[i]);
  }
  const uint32_t* sl = kn.split_l;              // BP_NTT_SPLIT: the widths must add up to k, each <= 10
  if (kn.split_k == k && k > (uint32_t)NTT_SMALL_MAX_LOG && sl[0] + sl[1] + sl[2] == k && sl[0] >= 2 && sl[1] >= 1 &&
      sl[0] <= (uint32_t)NTT_MAX_PASS_LOG && sl[1] <= (uint32_t)NTT_MAX_PASS_LOG && sl[2] <= (uint32_t)NTT_MAX_PASS_LOG) {
    P = sl[2] ? 3 : 2;
    for (uint32_t i = 0; i < 3; i++) l[i] = sl[i], cl[i] = i < P ? ntt_tile_cols_log(l[i]) : 0;
  }
  NttHostPlan p = {{k, P, {l[0], l[1], l[2], 0}, {cl[0], cl[1], cl[2], 0}, (k + 1) / 2}, {}, k <= kn.full_twiddles_max_log};
  for (uint32_t i = 0, s = k; i < P; i++) {
    s -= l[i];                                // bits below this digit
    p.pass[i] = P == 1 ? ntt_small_pass(k) : ntt_pass(k, l[i], i + 1 < P ? s : 0, cl[i], kn);
  }
  return p;
}
// The plan of a 2^k-point transform (the driver runs k <= 28).  An override (any knob) that gives an invalid plan is ignored as a whole: the default
// plan is used, the rule knob_u32 states for a malformed value.
inline NttHostPlan ntt_plan(uint32_t k, const NttKnobs& kn) {
  if (k > 3 * (uint32_t)NTT_MAX_PASS_LOG) return {{k, 0, {0, 0, 0, 0}, {0, 0, 0, 0}, 0}, {}, false};      // no passes: the driver refuses it
  const NttHostPlan p = ntt_plan_unchecked(k, kn);
  if (ntt_plan_valid(p)) return p;
  NttKnobs dflt;
  dflt.full_twiddles_max_log = kn.full_twiddles_max_log;       // (not a knob of the plan's shape)
  return ntt_plan_unchecked(k, dflt);
}

// One transform cut in two phases for a group context (NTT option ii; capi_ntt.hip ntt_one_over_members): with the
// digits N = 2^(l_1 + s), phase 0 is pass 1 on the tiles of a COLUMN slice (all d_1, r in the part's range), phase 1 the passes
// 2 .. P on the slice of e_1 (each e_1 owns 2^s contiguous elements of the intermediate buffer).  Between the phases the members
// exchange blocks of the intermediate buffer.  Every member keeps buffers in the full N-element layout, so addresses are the
// single-GPU ones and a part is just a range of tiles: [part, part + 1) * tiles / parts in every pass (e_1 is the most
// significant part of every later pass's tile index).
inline bool ntt_split_ok(const NttHostPlan& p, uint32_t parts) {
  if (p.dev.P < 2 || parts < 2 || (parts & (parts - 1)) || parts > 8) return false;
  uint32_t lg = 0;
  while ((1u << lg) < parts) lg++;
  return p.pass[0].s >= p.pass[0].cl + lg &&                     // pass 1: whole tiles of columns per part
         p.pass[0].l >= p.pass[p.dev.P - 1].cl + lg;             // last pass: whole tiles of e_1 per part
}

}  // namespace bp

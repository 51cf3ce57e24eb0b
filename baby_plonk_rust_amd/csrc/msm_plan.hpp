// msm_plan.hpp -- everything the G1 MSM decides from numbers alone: the kernels' limits, the struct that travels to them (MsmPlan), the
// experiment knobs and the plan of one pipeline (window width, digit radix, sort and record form, slices, launch shapes, the bucket tree,
// every workspace size), validated as a whole.  Host-pure: no HIP runtime call and no bp_ctx; msm.hip plans, allocates and launches by
// what stands here, tests/test_msm_plan.py compiles it for the host alone and enumerates it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/bp_msm_ntt.h"      // BP_ERR_*
#include "msm_digits.hpp"

namespace bp {

// ---- limits shared by the kernels of msm_kernels.hpp and the plan
constexpr int MSM_MAX_C = 16;            // per-window bucket sets (any point set): one LDS histogram per window
constexpr int MSM_MAX_TABLE_C = 24;      // fixed-base tables: partitioned counting sort above 16 bits
constexpr uint32_t MSM_HIST_LOG = 15;    // buckets per LDS histogram (128 KiB of the 160)
constexpr int MSM_MAX_WINDOWS = 128;
constexpr uint32_t MSM_MAX_BATCH = 4;    // scalar vectors in one pipeline (MsmScalars)
constexpr int MSM_SLOTS = 4;             // result areas of a context's pinned staging buffer: its MSMs in flight together
constexpr uint32_t SCAN_TILE = 4096;     // counts per workgroup of the scan_* kernels
constexpr uint32_t RADIX_SLICE = 8192;   // records per workgroup pass of msm_radix_count / _scatter
constexpr uint32_t PART_MAX_BITS = 12, PART_MAX = 1u << PART_MAX_BITS;      // partitions of msm_part_count / _scatter
// a bucket cut into FIXUP_LONG chunks or more is queued for msm_fixup_long; one of more than FIXUP_LONG_SPLIT_FROM partials is summed by
// FIXUP_LONG_SLICES workgroups
constexpr uint32_t FIXUP_LONG = 16, FIXUP_LONG_SLICES = 8, FIXUP_LONG_SPLIT_FROM = 2048;
constexpr uint32_t PLANES_STEP_LOG = 6;  // tree levels per launch of msm_planes_step
constexpr uint32_t MSM_SLOT_BYTES = 176; // sizeof(proj28_slot): an accumulator in HBM (msm.hip asserts the match)
// dynamic-LDS limits per kernel: msm_init_device sets them (hipFuncSetAttribute), msm_plan_valid holds every request against them.
// msm_radix_scatter and msm_radix_final / _long_* also hold a few KiB of static LDS: the dynamic limit leaves room for it.
constexpr size_t MSM_LDS_RADIX_SCATTER = 96 * 1024;      // msm_radix_scatter
constexpr size_t MSM_LDS_RUN_HIST = 144 * 1024;          // msm_radix_final, msm_radix_long_count, msm_radix_long_scatter
constexpr size_t MSM_LDS_PART_SCATTER = 156 * 1024;      // msm_part_scatter
constexpr size_t MSM_LDS_DEFAULT = 64 * 1024;            // every other kernel (msm_fixup_long, msm_planes_step): no attribute set

struct MsmPlan {
  uint32_t n;          // number of (point, scalar) pairs
  uint32_t c;          // window bits
  uint32_t W;          // windows
  uint32_t B;          // buckets per window = 2^(c-1)
  uint32_t chunk;      // entries per lane in msm_accumulate when every digit is non-zero (sizes the lane count and the partial slots)
  uint32_t lanes;      // 0: the chunk is fixed (BP_MSM_CHUNK).  Else the lanes of msm_accumulate = ceil(W n / chunk): the kernels cut
                       // the sorted list into ceil(M / lanes) entries per lane from the ACTUAL entry count M (zero digits are
                       // not entries: small or sparse scalars keep every lane busy with short chains instead of a few lanes with long ones)
  uint32_t bias[9];    // sum_{w < W-1} 2^(c-1) * 2^(c*w)   (the top window is unsigned)
  // Two bucket layouts share every kernel.  Per-window buckets (any point set): window w owns buckets
  // [w B, (w+1) B) and an entry is the point index i.  Fixed-base tables (bp_srs_precompute): the SRS carries
  // T[w][i] = 2^(cw) P_i, every window feeds the SAME B buckets and an entry is the table index w * stride + i,
  // so the reduction and the Horner epilogue run over one window instead of W.
  uint32_t total;      // number of buckets: W * B, or B with tables
  uint32_t wbuckets;   // bucket-index stride per window: B, or 0 with tables
  uint32_t wpoints;    // point-index stride per window: 0, or the table row length with tables
  // Windows wider than 16 bits (fixed-base tables only): one window's 2^(c-1) buckets no longer fit one LDS histogram
  // (parts > 1); those MSMs take the partitioned (radix) bucket sort, section 4c.
  uint32_t parts;      // 1, or B >> 15
  // Several scalar vectors against ONE table set in one pipeline (the commitments of a prover round, prover.rs:249-251,
  // 483-485, 640-641): vector j owns the buckets [j B, (j + 1) B), so the sort, the accumulation, the fix-up and the tree run
  // once over J bucket sets and deliver J results.  n is then the longest vector; scalar (j, i) is element j * n + i of the
  // pipeline's index space, elements with i >= nj[j] do not exist.  Partition sort only (msm_part_*); J = 1 everywhere else.
  uint32_t J;          // 1 .. MSM_MAX_BATCH
  uint32_t nj[4];      // length of vector j
  // Fixed-base tables free the digit radix from being a power of two (round 6): T[w][i] = R^w P_i for ANY R.  W windows of c bits cover
  // c W >= 256 bits, but a scalar has 255: at c = 20 (13 windows) five bits of every bucket index are bought and never used.  With
  // R = the smallest (low Hamming weight) even number whose W-th power exceeds 2^256 the signed digits |d| <= R / 2 fill R / 2 buckets
  // instead of 2^(c-1): 425 984 instead of 524 288 at 13 windows, 1 327 104 instead of 2 097 152 at 12 -- a fifth to a third of the
  // bucket tree's leaves (and of its additions) gone; the live buckets are a PREFIX of the 2^(c-1) the tree is sized for, the rest
  // stay empty and whole waves of the tree skip them.  radix = 0: power-of-two windows (every table-free MSM; widths that waste < 10 %).
  // Digits: k' = k + bias (bias = sum_{w < W-1} (R / 2) R^w), f = k' / R^W as a 288-bit fraction = the top limbs of k' * radix_m
  // (radix_m = ceil(2^512 / R^W)) + 2 ulp, then W times "multiply by R, take the integer part" from the top digit down; signed digit
  // = that - R / 2 below the top window.  Exact: the fraction's error is in [0, 2^-257 + 2^-287) and 1 / R^W > 2^-256.93 (msm_digits.hpp).
  uint32_t radix;
  uint32_t radix_m[8];
};

// ---- the experiment knobs (BP_MSM_*).  The initialisers are the shipped behaviour; msm.hip's msm_knobs() fills the
// struct from the environment in the experiment build, on every call.  0 / 99 = not set where the driver tells that from every value.
struct MsmKnobs {
  uint32_t c = 0;                      // BP_MSM_C, 2..16: window width of a table-free MSM; 0: from n
  uint32_t chunk = 0;                  // BP_MSM_CHUNK, 1..1024: a fixed chunk, MsmPlan::lanes off; 0: the chunk rounds below, lanes on
  uint32_t radix = 1;                  // BP_MSM_RADIX, 0 / 1: 0 keeps power-of-two windows everywhere
  uint32_t radix_from = 21;            // BP_MSM_RADIX_FROM, 8..30: narrowest table width that takes its radix
  uint32_t radix_bits = 99;            // BP_MSM_RADIX_BITS, 0..16: partition bits pb asked for; 99: by run length (and the packed rule may raise it)
  uint32_t packed = 1;                 // BP_MSM_PACKED, 0..2: 0 two-word records, 1 one word where it fits (raising pb for it), 2 one word at the run length's pb
  uint32_t sort = 2;                   // BP_MSM_SORT, 1 / 2: 1 forces the two-level sort
  uint32_t part_slice = 0;             // BP_MSM_PART_SLICE, 64..4096: scalars per workgroup of msm_part_scatter; 0: part_slice below
  uint32_t part_wide8 = 1;             // BP_MSM_PART_WIDE8, 0 / 1: 0 keeps 512-scalar slices for two-word records
  uint32_t count_slice = 0;            // BP_MSM_COUNT_SLICE, 64..65536: scalars per workgroup of msm_part_count; 0: part_slice below
  uint32_t part_flat = 2;              // BP_MSM_PART_FLAT, 0..2: 0 partition-major write-out, 1 one lane per record, 2 by the slice's share of a partition
  uint32_t final_threads = 0;          // BP_MSM_FINAL_THREADS, 256..1024: lanes of msm_radix_final (partition sort); 0: by run length
  uint32_t fixup = 0;                  // BP_MSM_FIXUP, 0..2: 1 per bucket, 2 per chunk edge, 0 by entries per bucket
  uint32_t planes_wide_min = 24000;    // BP_MSM_PLANES_WIDE_MIN, 256..2^30: additions from which a tree level runs one per lane
};

// the variables and their ranges: get(name, default, lo, hi) answers the default for a value that is absent, malformed or outside [lo, hi]
// (knob_u32 of ctx.hpp, in msm.hip's msm_knobs())
template <class Get>
inline MsmKnobs msm_knobs_read(Get&& get) {
  MsmKnobs kn;
  kn.c = get("BP_MSM_C", kn.c, 2, MSM_MAX_C);
  kn.chunk = get("BP_MSM_CHUNK", kn.chunk, 1, 1024);
  kn.radix = get("BP_MSM_RADIX", kn.radix, 0, 1);
  kn.radix_from = get("BP_MSM_RADIX_FROM", kn.radix_from, 8, 30);
  kn.radix_bits = get("BP_MSM_RADIX_BITS", kn.radix_bits, 0, 16);
  kn.packed = get("BP_MSM_PACKED", kn.packed, 0, 2);
  kn.sort = get("BP_MSM_SORT", kn.sort, 1, 2);
  kn.part_slice = get("BP_MSM_PART_SLICE", kn.part_slice, 64, 4096);
  kn.part_wide8 = get("BP_MSM_PART_WIDE8", kn.part_wide8, 0, 1);
  kn.count_slice = get("BP_MSM_COUNT_SLICE", kn.count_slice, 64, 65536);
  kn.part_flat = get("BP_MSM_PART_FLAT", kn.part_flat, 0, 2);
  kn.final_threads = get("BP_MSM_FINAL_THREADS", kn.final_threads, 256, 1024);
  kn.fixup = get("BP_MSM_FIXUP", kn.fixup, 0, 2);
  kn.planes_wide_min = get("BP_MSM_PLANES_WIDE_MIN", kn.planes_wide_min, 256, 1u << 30);
  return kn;
}

// ---- window count and digit radix of a width
struct MsmWidth {
  uint32_t W = 0;
  uint32_t bias[9] = {0};      // power-of-two windows: sum_{w < W-1} 2^(c-1) 2^(cw)
  MsmRadix radix;              // msm_radix_compute(c, W): what fixed-base tables of this width may cut instead (R = 0: nothing to gain)
};
inline MsmWidth msm_width_compute(uint32_t c) {
  // Windows 0..W-2 are signed: d_w = ((k + bias) >> cw & mask) - 2^(c-1), bias = sum_{w<W-1} 2^(c-1) 2^(cw).
  // The top window is unsigned (digit = remaining high bits, carry included) and must fit a bucket index,
  // i.e. be <= 2^(c-1) for every k < q.  Smallest such W, from ceil(255 / c) up, checked with the real q:
  static const uint32_t q_minus_1[8] = {0x00000000u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
  MsmWidth out;
  uint32_t W = (255 + c - 1) / c;
  if (W < 2) W = 2;
  for (;; W++) {
    uint32_t bias[10] = {0};
    for (uint32_t w = 0; w + 1 < W; w++) {
      const uint32_t bit = c * w + c - 1;
      if (bit < 320) bias[bit >> 5] |= 1u << (bit & 31);
    }
    uint64_t carry = 0;
    uint32_t sum[11] = {0};
    for (int j = 0; j < 10; j++) {
      carry += (uint64_t)(j < 8 ? q_minus_1[j] : 0u) + bias[j];
      sum[j] = (uint32_t)carry;
      carry >>= 32;
    }
    // top digit of the largest scalar: (q - 1 + bias) >> c (W - 1), as an exact 320-bit shift
    const uint32_t o = c * (W - 1);
    bool ok = o < 288;
    uint64_t top = 0;
    for (int bit = 319; bit >= (int)o && ok; bit--) {
      if ((sum[bit >> 5] >> (bit & 31)) & 1) {
        if (bit - (int)o >= 32) ok = false; else top |= 1ull << (bit - o);
      }
    }
    if (ok && top <= (1ull << (c - 1))) {
      memcpy(out.bias, bias, sizeof out.bias);
      break;
    }
  }
  out.W = W;
  out.radix = msm_radix_compute(c, W);
  return out;
}
// cached for every width a plan can take, 2 <= c <= MSM_MAX_TABLE_C: planning is on the host's hot path of a half-millisecond MSM
inline const MsmWidth& msm_width(uint32_t c) {
  struct Table {
    MsmWidth w[MSM_MAX_TABLE_C + 1];
    Table() { for (uint32_t c = 2; c <= (uint32_t)MSM_MAX_TABLE_C; c++) w[c] = msm_width_compute(c); }
  };
  static const Table table;
  return table.w[c];
}
inline uint32_t msm_windows(uint32_t c) { return msm_width(c).W; }      // = rows of the fixed-base tables of width c
// Radix of the tables of width c (0: power-of-two windows), from 21 bits only (2^20 allocated buckets and more).  Fewer live buckets save
// tree time only where a tree level runs for several wave rounds: at c = 22 (2^21 buckets, 2^24 points) the radix takes 0.3 ms off the
// 5.3-ms tail and 0.65 ms off the MSM; at c = 20 every wide level of the 2^19-bucket tree is ONE round of two waves per SIMD, a fifth of
// the workgroups leaving early frees no SIMD earlier, and the division costs msm_part_count 9 us: 2.60-2.64 against 2.63 ms, no gain
// (profiles/r06_tail_ab.txt).  Experiment build: BP_MSM_RADIX=0 keeps power-of-two windows everywhere, BP_MSM_RADIX_FROM moves the threshold.
inline const MsmRadix* msm_table_radix(uint32_t c, const MsmKnobs& kn) {
  return kn.radix != 0 && c >= kn.radix_from && msm_width(c).radix.R ? &msm_width(c).radix : nullptr;
}

// ---- width of the fixed-base tables of an SRS
// tables of width c pay for an MSM of n points once the bucket adds outweigh the fixed 2^c reduction
inline bool srs_width_pays(uint32_t c, size_t n) { return 8 * (uint64_t)n >= (1ull << c); }
// the automatic width (bp_srs_precompute with window_bits = 0), from the length of one shard
inline uint32_t srs_auto_width(uint64_t n) {
  uint32_t lg = 0;
  while ((2ull << lg) <= n) lg++;                        // floor(log2 n)
  if (lg >= 24) return 22;          // 12 windows: the 2^21-bucket tree (+0.8 ms) against n fewer additions (-1.8 ms at 2^24; a tie at 2^23)
  // 13 windows instead of 16: pays once the sort and the 2^19-bucket tree are small against 3 x n additions (round 3: -3 % at 2^20,
  // -6 % at 2^21, -12 % at 2^22; profiles/r03_window_width_ab.txt)
  if (lg >= 20) return 20;
  if (n >= (1u << 14)) return lg + 2 > 16 ? 16 : lg + 2;      // throughput regime: reduction work 2^c stays below the bucket-add work W * n
  // latency regime (a few thousand points): every kernel is a dependent chain, and the reduction tree has c - 1 levels -- measured
  // optimum 2^10: 6, 2^12: 8
  return lg > 8 ? lg - 4 : 4;
}

// ---- the plan of one pipeline
// msm_part_count + msm_part_scatter cutting 2^pb partitions straight from the scalars: the partition sort, or level 1 of the two-level sort
struct MsmLevel1 {
  uint32_t pb, rb;                    // partition bits and the bucket bits below them
  uint32_t slice, n_slices;           // scalars per workgroup of msm_part_scatter, its grid
  uint32_t slice1, n_slices1;         // the same of msm_part_count
  uint32_t count_threads, scatter_threads;
  uint32_t cap;                       // records a scatter workgroup stages: slice * W
  size_t part_lds;                    // dynamic LDS of msm_part_scatter
};
enum : uint8_t { MSM_STEP_LEVEL01, MSM_STEP_LEVEL, MSM_STEP_STEP };      // msm_planes_level01 / msm_planes_level / msm_planes_step
enum : uint8_t { MSM_OUT_TMP0, MSM_OUT_TMP1, MSM_OUT_FINAL };            // msm.planes_tmp0 / _tmp1 / where the epilogue reads (window_sum or roots)
struct MsmTreeStep {
  uint8_t kind, out;
  uint32_t k, m;                      // first level and number of levels of this launch
  uint32_t nodes;                     // nodes it leaves, each of k + m + 1 values
  uint32_t gx, gy, lds;               // grid and dynamic LDS (block: 256)
};
constexpr uint32_t MSM_MAX_TREE_STEPS = MSM_MAX_TABLE_C;
// named device workspaces, in bytes (0: not used by this pipeline)
struct MsmWsBytes {
  size_t ctl, counts, offsets, cursors, long_list, long_scratch, tile_sums, sorted, bucket_sum, partial, roots, window_sum;
  size_t rkeys0, rvals0, rkeys1, rvals1, run_off, run_cnt, run_cur, run_long, planes_tmp0, planes_tmp1;
};
struct MsmHostPlan {
  int err;                            // BP_OK, or the refusal: its code and text
  const char* what;
  bool empty;                         // no scalars: nothing to launch, every other field is zero
  MsmPlan dev;                        // what travels to the kernels
  uint64_t entries, n_chunks;         // W * n * J, and ceil(entries / chunk): the lanes of msm_accumulate
  uint32_t kb, pb, rbits, vb;         // bits of a bucket id, partition bits, bucket bits of a final run, bits of an entry + sign
  uint32_t sort;                      // 1 two-level, 2 partition
  bool packed, flat, wide8;           // partition sort: one-word records, one lane per record in the write-out, 1 024-scalar slices of two-word records
  MsmLevel1 l1;
  // the second level of the two-level sort (lv[1] = 0: none): msm_radix_count / scan_* / msm_radix_scatter cut each of the 2^lv[0] runs by lv[1] bits
  uint32_t lv[2], gx2, n_sub, shift2, scan_tiles;
  // final runs: msm_radix_final on final_grid workgroups of final_threads lanes; msm_radix_long_* on long_gx x long_gy (0: a single run, none)
  uint32_t n_final, final_grid, final_threads, long_gx, long_gy;
  size_t rhist;                       // dynamic LDS of the three: one run's bucket histogram
  // control words, zeroed by ONE memset per MSM: [0] long-bucket counter, [1] scalar status, [2] long-run counter of the sort,
  // [4] ticket + [5 ..] partition sizes of msm_part_count, [8 + PART_MAX ..] one ticket per queued long bucket (msm_fixup_long),
  // [run_ticket ..] one ticket per long RUN of the sort (msm_radix_long_count; at most 2^16 final runs).  The memset covers the words in use.
  uint32_t long_cap, ctl_words, ctl_zeroed, run_ticket;
  uint32_t acc_grid;
  bool by_edges;                      // fix-up per chunk edge (msm_fixup_edges); else per bucket (msm_fixup<2> with tables, <1> without)
  uint32_t fixup_grid;
  uint32_t quads, per_window, n_planes, Wr;      // values per window for the host, slots per window, slots in all, bucket sets left after accumulation
  uint32_t n_wide, n_steps;           // tree levels that run one addition per lane; launches of the tree
  MsmTreeStep step[MSM_MAX_TREE_STEPS];
  size_t tmp_slots[2];                // accumulator slots of msm.planes_tmp0 / _tmp1
  MsmWsBytes ws;
};

// scalars per workgroup of a pass that cuts digits from the scalars: `slice` doubled up to `limit` while that leaves at least `wgs` workgroups
// and the pass's staging area (`staged` bytes per scalar, twice) stays within 64 KiB
inline uint32_t part_slice(uint32_t slice, uint32_t limit, uint32_t wgs, uint64_t scalars, uint64_t staged) {
  while (slice < limit && 2 * slice * staged <= 65536 && (uint64_t)slice * wgs < scalars) slice <<= 1;
  return slice;
}
inline uint32_t msm_ceil_div(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

// level 1 behind its slice: the count pass keeps nothing per slice, so its slices are its own: fatter ones (~256 workgroups) flush their
// 2^pb partition sizes with a quarter of the global atomics (measured at 2^20: 48 / 41 / 34 / 48 us at 1 024 / 2 048 / 4 096 / 8 192)
inline MsmLevel1 msm_level1(uint32_t slice, uint32_t count_slice, uint64_t scalars, uint32_t W, uint32_t pb, uint32_t rb) {
  MsmLevel1 s = {pb, rb, slice, msm_ceil_div(scalars, slice), 0, 0, 0, 0, slice * W, 0};
  s.scatter_threads = slice >= 1024 ? 1024u : (slice <= 256 ? 256u : slice);
  s.slice1 = count_slice ? count_slice : part_slice(slice, 8192, 256, scalars, 0);
  s.n_slices1 = msm_ceil_div(scalars, s.slice1);
  s.count_threads = s.slice1 >= 1024 ? 1024u : s.scatter_threads;
  return s;
}

// The plan of J scalar vectors of n_each[j] scalars against one point set: table_c != 0 when the points are fixed-base window tables of
// that width with rows table_stride apart (J > 1: tables only, and no record in HBM).  A function of its arguments alone.
inline MsmHostPlan msm_plan(uint32_t J, const size_t* n_each, uint32_t table_c, size_t table_stride, bool blob, const MsmKnobs& kn) {
  MsmHostPlan hp;
  memset(&hp, 0, sizeof hp);
  auto refuse = [&hp](int code, const char* what) -> MsmHostPlan& { hp.err = code; hp.what = what; return hp; };
  if (J < 1 || J > MSM_MAX_BATCH || (J > 1 && (!table_c || blob))) return refuse(BP_ERR_INVALID_ARG, "MSM batch");
  if (table_c > (uint32_t)MSM_MAX_TABLE_C) return refuse(BP_ERR_INVALID_ARG, "MSM table width");      // (bp_srs_precompute builds 4..24)
  size_t n = 0;
  for (uint32_t j = 0; j < J; j++) n = n_each[j] > n ? n_each[j] : n;
  if (n == 0) {
    hp.empty = true;
    return hp;
  }
  if (n >= (1ull << 31)) return refuse(BP_ERR_TOO_LARGE, "MSM length >= 2^31");
  // Window width: minimise W * (n + 2 * 2^(c-1)) (bucket adds + reduction adds).  Per-window bucket sets (any point set) are
  // bounded by the 128 KiB LDS histogram of one window (c <= 16); with fixed-base tables wider windows go through the
  // partitioned sort (plan.parts > 1), up to MSM_MAX_TABLE_C.
  MsmPlan& plan = hp.dev;
  uint32_t lg = 0;
  while ((n >> (lg + 1)) != 0) lg++;
  uint32_t c = n < 32 ? 4 : lg - 3;
  if (c < 4) c = 4;
  if (c > (uint32_t)MSM_MAX_C) c = MSM_MAX_C;
  if (kn.c) c = kn.c;
  if (table_c) c = table_c;
  if (c < 2) c = 2;
  const MsmWidth& width = msm_width(c);
  const MsmRadix* rx = table_c ? msm_table_radix(c, kn) : nullptr;      // fixed-base tables: the radix need not be a power of two
  const uint32_t W = width.W;
  plan.n = (uint32_t)n;
  plan.J = J;
  for (uint32_t j = 0; j < J; j++) plan.nj[j] = (uint32_t)n_each[j];
  plan.c = c;
  plan.W = W;
  plan.B = 1u << (c - 1);
  memcpy(plan.bias, rx ? rx->bias : width.bias, sizeof plan.bias);
  if (rx) {
    plan.radix = rx->R;
    memcpy(plan.radix_m, rx->m, sizeof plan.radix_m);
  }
  plan.total = table_c ? J * plan.B : W * plan.B;
  plan.wbuckets = table_c ? 0 : plan.B;
  plan.wpoints = table_c ? (uint32_t)table_stride : 0;
  plan.parts = plan.B <= (1u << MSM_HIST_LOG) ? 1 : plan.B >> MSM_HIST_LOG;
  const uint64_t entries = (uint64_t)W * n * J;
  if (entries >= (1ull << 32)) return refuse(BP_ERR_TOO_LARGE, "MSM length * windows >= 2^32");      // positions in the bucket-sorted list are 32-bit
  // entries per lane: the kernel runs 2 waves per SIMD = 131072 lanes at a time and every lane does the same work, so the
  // lane count should land just under a whole number of such rounds.  (A power-of-two chunk wasted up to a third of the last
  // round whenever windows * n was not a power of two: 13 or 15 windows.)  Measured with tables (r02_chunk_rounds_ab.txt):
  //   up to 2^20 entries (2^16 points): half a round -- chains of 16 leave two partials per bucket instead of eight (0.531 -> 0.482 ms);
  //   up to 2*10^7 entries (2^20 points and the prover's 2^20 + 6): ONE round (2^20: 3.13 -> 3.03 ms, 2^18 1.004 -> 0.979, 2^17 0.723 -> 0.675);
  //   beyond: two rounds (2^21 .. 2^24 are equal or 1-3 % better with two: the second round evens out the lanes' finish times).
  // Per-window buckets (no tables) are short: cap the chunk at 64.
  const uint32_t chunk_cap = table_c ? 1024u : 64u;
  uint32_t chunk;
  if (table_c && entries <= (1u << 20)) chunk = (uint32_t)(entries >> 16);
  else if (table_c && entries <= 20000000u) chunk = msm_ceil_div(entries, 131072);      // 2^24 and a little more: the prover's SRS has n + 6 points
  else chunk = msm_ceil_div(entries, 262144);
  if (chunk < 4) chunk = 4;
  if (chunk > chunk_cap) chunk = chunk_cap;
  plan.chunk = kn.chunk ? kn.chunk : chunk;
  hp.entries = entries;
  hp.n_chunks = (entries + plan.chunk - 1) / plan.chunk;
  plan.lanes = kn.chunk ? 0u : (uint32_t)hp.n_chunks;
  const uint32_t total = plan.total;
  // Bucket reduction: the bit-plane tree over one bucket set (tables) or, without tables, over the forest of the W bucket sets of 2^(c-1)
  // buckets (running sums per window, a dependent chain of ~46 additions per lane, cost 0.57 ms at 2^20 points: docs/EXPERIMENTS.md Q), then
  // two levels of the Horner form over each tree's c values (msm_planes_window_quads): `quads` values per window go to the host.
  hp.Wr = table_c ? J : W;
  hp.quads = table_c ? 1u : (c + 2) / 4;              // ceil((c - 1) / 4); c = 2: one quad (A + T_0)
  hp.per_window = table_c ? c : hp.quads;
  hp.n_planes = hp.Wr * hp.per_window;                // tables: A and the c - 1 bit planes; else one sum per window
  if (hp.n_planes > (uint32_t)MSM_MAX_WINDOWS) return refuse(BP_ERR_TOO_LARGE, "MSM windows");
  // a bucket is "long" when it spans >= FIXUP_LONG chunks, so at most n_chunks / FIXUP_LONG + 1 buckets can be long
  hp.long_cap = (uint32_t)(hp.n_chunks / FIXUP_LONG + 1);

  // ---- bucket sort, two builds: the partition sort (default wherever its 2^pb <= 2^11 partitions leave final runs
  // that one workgroup sorts: up to ~5 * 10^7 entries) and the two-level radix sort (beyond; BP_MSM_SORT=1 forces it, 2 is the default).
  uint32_t kb = 0;
  while ((1ull << kb) < total) kb++;
  uint32_t pb = 0;
  // final runs of ~12-24 Ki entries; per-window bucket sets (no tables) take runs of half that length: 2^9 buckets of 16 entries per run sort
  // faster than 2^9 buckets of 32 (tail 0.84 -> 0.80 ms at 2^20, 0.83 -> 0.80 at 2^18, 0.63 -> 0.60 at 2^16: tools/part_bits_probe.sh, round 5)
  const uint64_t run_min = table_c ? 12288 : 6144;
  while (pb < kb && (entries >> (pb + 1)) >= run_min) pb++;
  if (kn.radix_bits != 99) pb = kn.radix_bits;
  if (pb + MSM_HIST_LOG < kb) pb = kb - MSM_HIST_LOG;                   // a final run's buckets must fit one LDS histogram
  if (pb > kb) pb = kb;
  if (pb > 16) pb = 16;
  if (pb > PART_MAX_BITS && (entries >> PART_MAX_BITS) <= 32768) pb = PART_MAX_BITS;     // final runs of up to 32 Ki entries are fine for one workgroup
  if (pb + MSM_HIST_LOG < kb) pb = kb - MSM_HIST_LOG;
  // record form of the partition sort: the packed word holds the bucket's low kb - pb bits, the sign and the entry (point or
  // table index, vb - 1 bits).  Where a few more partitions make the record fit one word (c = 20 at 2^20: 2^12 instead of 2^10)
  // they are taken: half the bytes through the scatter and the final sort (BP_MSM_PACKED=2 keeps the run length instead).
  const uint64_t idx_max = (uint64_t)(n - 1) + (uint64_t)(W - 1) * plan.wpoints;
  uint32_t vb = 1;
  while ((idx_max >> (vb - 1)) != 0) vb++;                              // vb - 1 = bits of the largest entry, + 1 for the sign
  if (kn.packed == 1 && kb + vb > 32 + pb && kb + vb - 32 <= PART_MAX_BITS && kn.radix_bits == 99) pb = kb + vb - 32;
  // 1: the two-level sort.  BP_MSM_SORT=1 takes it at sizes where the partition sort is the default (pb = 0 leaves no level to sort by: ignored)
  hp.sort = ((kn.sort == 1 && J == 1 && pb > 0) || pb > PART_MAX_BITS) ? 1 : 2;
  if (hp.sort != 2 && J > 1) return refuse(BP_ERR_TOO_LARGE, "MSM batch too long for the partition sort");
  const uint32_t rbits = kb - pb, n_final = 1u << pb;
  hp.kb = kb, hp.pb = pb, hp.rbits = rbits, hp.vb = vb, hp.n_final = n_final;
  hp.rhist = ((size_t)1 << rbits) * 4;
  hp.final_grid = n_final < 4096 ? n_final : 4096;
  const uint64_t scalars = (uint64_t)n * J;
  if (hp.sort == 2) {
    hp.packed = rbits + vb <= 32 && kn.packed != 0;
    const uint32_t rec_bytes = hp.packed ? 4 : 8;
    // scalars per workgroup: the staging area (slice * W records) within 64 KiB, and >= 512 workgroups where n allows
    uint32_t slice = kn.part_slice ? kn.part_slice : part_slice(64, 1024, 512, scalars, (uint64_t)W * rec_bytes);
    if ((uint64_t)slice * W * rec_bytes > 65536) slice = 64;
    // Two-word records (2^21 .. 2^23 points at c = 20: bucket-low bits + sign + a 25..27-bit table index exceed one word): the 64-KiB rule leaves
    // slices of 512 scalars, and a workgroup's fixed cost for its 2^12-entry tables (~12 us) then outweighs its records (~7 us).  A slice of
    // 1 024 scalars stages 104 KiB; that fits beside the 48 KiB of tables when the per-record partition array of the flat write-out is dropped,
    // i.e. with the partition-major write-out (BP_MSM_PART_WIDE8=0 keeps the 512-scalar slices).
    hp.wide8 = !hp.packed && slice == 512 && (uint64_t)1024 * 512 < scalars && (size_t)3 * n_final * 4 + (size_t)1024 * W * 8 <= MSM_LDS_PART_SCATTER &&
               kn.part_wide8 != 0;
    if (hp.wide8) slice = 1024;
    hp.l1 = msm_level1(slice, kn.count_slice, scalars, W, pb, rbits);
    // a slice's share of a partition: long -> partition-major write-out, short -> one lane per record (BP_MSM_PART_FLAT = 0 / 1 forces)
    hp.flat = hp.wide8 ? false : (kn.part_flat == 2 ? (hp.l1.cap >> pb) < 8 : kn.part_flat == 1);
    hp.l1.part_lds = (size_t)3 * n_final * 4 + (size_t)hp.l1.cap * rec_bytes + (hp.flat ? (size_t)hp.l1.cap * 2 : 0);
    // short final runs (2^12 runs of ~3 Ki records at c = 20): 512-lane workgroups (measured 70 / 60 / 72 us at 256 / 512 / 1024 lanes)
    hp.final_threads = (kn.final_threads ? kn.final_threads : ((entries >> pb) <= 8192 ? 512u : 1024u)) & ~63u;
    if (n_final > 1) hp.long_gx = 64, hp.long_gy = n_final < 4 ? n_final : 4;
  } else {
    // Level 1 comes straight from the scalars, as the partition sort does it (msm_part_count + msm_part_scatter with two-word records into
    // 2^lv[0] runs: no record pass, one array's traffic less -- 2^24 points, tail 5.87 -> 5.32 ms, profiles/r04_sort24_hybrid_ab.txt).
    hp.lv[0] = pb <= 8 ? pb : pb - pb / 2;
    hp.lv[1] = pb <= 8 ? 0 : pb / 2;
    const uint32_t pb1 = hp.lv[0], rb1 = kb - pb1, runs = 1u << pb1;
    hp.l1 = msm_level1(part_slice(64, 1024, 512, scalars, (uint64_t)W * 8), 0, scalars, W, pb1, rb1);
    hp.l1.part_lds = (size_t)3 * runs * 4 + (size_t)hp.l1.cap * 8;
    if (hp.lv[1]) {                 // the second level: msm_radix_count / _scatter cut each run of level 1 by the next lv[1] bits
      hp.n_sub = runs << hp.lv[1];
      hp.shift2 = rb1 - hp.lv[1];
      const uint64_t gx = (entries / runs + RADIX_SLICE - 1) / RADIX_SLICE + (runs > 1 ? 1 : 0);
      hp.gx2 = gx > 4096 ? 4096u : (uint32_t)gx;
      hp.scan_tiles = msm_ceil_div(hp.n_sub, SCAN_TILE);
    }
    hp.final_threads = 1024;
    if (n_final > 1) hp.long_gx = 256, hp.long_gy = n_final < 16 ? n_final : 16;      // long runs (none for uniformly random scalars beyond the top window's): slice-parallel
  }
  hp.run_ticket = 8 + PART_MAX + hp.long_cap;
  hp.ctl_words = hp.run_ticket + 65536;
  hp.ctl_zeroed = hp.run_ticket + n_final;

  hp.acc_grid = msm_ceil_div(hp.n_chunks, 256);
  // fix-up of the buckets cut by chunk edges.  Long buckets (tables at c <= 17: every one of the 2^15 buckets spans several chunks):
  // two lanes per bucket = one wave per SIMD, half the chain.  Short buckets (wide windows, per-window bucket sets): most buckets
  // sit inside one chunk -- one lane per chunk edge.  BP_MSM_FIXUP=1 / 2 forces the per-bucket / per-edge form.
  hp.by_edges = kn.fixup ? kn.fixup == 2 : entries / total < 2ull * plan.chunk;
  hp.fixup_grid = hp.by_edges ? hp.acc_grid : msm_ceil_div((uint64_t)total * (table_c ? 2 : 1), 256);

  // ---- the tree over the `total` leaves (tables: B = 2^(c-1) buckets, J B for a batch; table-free: the forest of W trees, W B leaves),
  // level by level.  A level with at least planes_wide_min additions is throughput bound: one addition per lane through HBM
  // (msm_planes_level01 / msm_planes_level: six such levels at 2^19 leaves, seven for the table-free forest of 16 x 2^15).  The rest
  // is latency bound: up to PLANES_STEP_LOG levels per launch inside workgroups, cooperative additions (msm_planes_step).
  // A node of 2^k buckets carries k + 1 values; the two ping-pong buffers hold at most B values (level 1).
  const uint32_t levels = c - 1;                        // >= 1
  uint32_t n_wide = 0;
  while (n_wide < levels && (uint64_t)(total >> (n_wide + 1)) * (n_wide + 1) >= kn.planes_wide_min) n_wide++;
  if (n_wide == levels) n_wide = levels - 1;            // the last level is always a step: it writes the result where the epilogue reads it
  // levels 0 and 1 have the same number of additions, so a wide level 0 comes with a wide level 1 and the two run fused (msm_planes_level01);
  // a lone wide leaf level (two-level trees, c = 3: knobs only) takes the step path
  if (n_wide < 2) n_wide = 0;
  hp.n_wide = n_wide;
  for (uint32_t k = 0, flip = 0; k < levels; flip ^= 1) {
    MsmTreeStep& s = hp.step[hp.n_steps++];
    s.k = k;
    if (k == 0 && n_wide) {               // levels 0 and 1 in one launch, four buckets per lane
      // msm.planes_tmp0 is sized as if level 0 wrote its output there; the fused launch does not, and no later level needs as much
      // (kept: this header changes no allocation -- without this line the buffer halves)
      hp.tmp_slots[0] = (size_t)(total >> 1) * 2;
      flip ^= 1;                          // the output takes the buffer level 1 would have taken
      s.kind = MSM_STEP_LEVEL01, s.m = 2;
      s.nodes = total >> 2;
      s.gx = msm_ceil_div(s.nodes, 256), s.gy = 1;
    } else if (k < n_wide) {
      s.kind = MSM_STEP_LEVEL, s.m = 1;
      s.nodes = total >> (k + 1);
      s.gx = msm_ceil_div((uint64_t)s.nodes * (k + 1), 256), s.gy = 1;
    } else {
      s.kind = MSM_STEP_STEP, s.m = levels - k < PLANES_STEP_LOG ? levels - k : PLANES_STEP_LOG;
      s.nodes = total >> (k + s.m);
      s.gx = s.nodes, s.gy = k + 1;
      s.lds = (2u << s.m) * MSM_SLOT_BYTES;
    }
    k += s.m;
    s.out = k == levels ? MSM_OUT_FINAL : (flip ? MSM_OUT_TMP1 : MSM_OUT_TMP0);
    const size_t slots = (size_t)s.nodes * (k + 1);
    if (s.out != MSM_OUT_FINAL && slots > hp.tmp_slots[flip]) hp.tmp_slots[flip] = slots;
  }

  MsmWsBytes& ws = hp.ws;
  ws.ctl = (size_t)hp.ctl_words * 4;
  ws.counts = (size_t)total * 4;                        // bucket sizes of the sort's long runs
  ws.offsets = ((size_t)total + 1) * 4;
  ws.cursors = (size_t)total * 4;
  ws.long_list = (size_t)hp.long_cap * 4;
  // slice sums of the buckets that take several workgroups: those have > FIXUP_LONG_SPLIT_FROM partials, so there are few of them, but the
  // slot is addressed by the bucket's place in the list
  ws.long_scratch = (size_t)hp.long_cap * FIXUP_LONG_SLICES * MSM_SLOT_BYTES;
  ws.tile_sums = 4096 * 4;
  ws.sorted = entries * 4;
  ws.bucket_sum = (size_t)total * MSM_SLOT_BYTES;
  ws.partial = 2 * hp.n_chunks * MSM_SLOT_BYTES;
  ws.roots = table_c ? 0 : (size_t)W * c * MSM_SLOT_BYTES;      // table-free: the W roots (A, T_0 .. T_{c-2}) in front of the per-window Horner pass
  ws.window_sum = (size_t)hp.n_planes * MSM_SLOT_BYTES + 16;    // + the status word
  ws.rkeys0 = entries * 4;
  ws.rvals0 = hp.packed ? 0 : entries * 4;
  ws.rkeys1 = ws.rvals1 = hp.sort == 1 ? entries * 4 : 0;
  ws.run_off = ((size_t)3 * n_final + 16) * 4;
  ws.run_cnt = hp.sort == 1 ? (size_t)n_final * 4 : 0;
  ws.run_cur = (size_t)n_final * 4;
  ws.run_long = ((size_t)n_final + 2) * 4;
  ws.planes_tmp0 = hp.tmp_slots[0] * MSM_SLOT_BYTES;
  ws.planes_tmp1 = hp.tmp_slots[1] * MSM_SLOT_BYTES;
  return hp;
}

// the words of bp_msm_last_path: J, c, W, radix, sort, pb, packed, flat, wide8, fixup (0 per bucket, 1 per edge), n_wide, chunk
inline void msm_plan_path(const MsmHostPlan& hp, uint32_t out[12]) {
  const uint32_t w[12] = {hp.dev.J, hp.dev.c, hp.dev.W, hp.dev.radix, hp.sort, hp.pb, hp.packed, hp.flat, hp.wide8, hp.by_edges, hp.n_wide, hp.dev.chunk};
  memcpy(out, w, sizeof w);
}

// what the kernels' index arithmetic needs of a plan that is to be launched (not refused, not empty)
inline bool msm_plan_valid(const MsmHostPlan& hp) {
  const MsmPlan& p = hp.dev;
  const MsmLevel1& s = hp.l1;
  auto threads_ok = [](uint32_t t) { return t != 0 && t % 64 == 0 && t <= 1024; };
  if (hp.err || hp.empty) return false;
  // every LDS request under its kernel's limit
  if (s.part_lds > MSM_LDS_PART_SCATTER || hp.rhist > MSM_LDS_RUN_HIST || (hp.lv[1] && (size_t)RADIX_SLICE * 9 > MSM_LDS_RADIX_SCATTER)) return false;
  if (!threads_ok(s.count_threads) || !threads_ok(s.scatter_threads) || !threads_ok(hp.final_threads)) return false;
  // a final run's buckets fit one histogram; one ticket word per final run; a packed record is one word
  if (hp.rbits > MSM_HIST_LOG || hp.pb > 16 || hp.pb + hp.rbits != hp.kb || ((uint64_t)1 << hp.kb) < p.total) return false;
  if (hp.n_final != 1u << hp.pb || s.pb > PART_MAX_BITS || s.pb + s.rb != hp.kb) return false;      // msm_part_count's partition sizes: PART_MAX words
  if (hp.packed && hp.rbits + hp.vb > 32) return false;
  if (hp.sort == 2 ? s.pb != hp.pb : (p.J != 1 || hp.lv[0] + hp.lv[1] != hp.pb || hp.lv[1] > 8)) return false;      // msm_radix_scatter: at most 256 digits
  // the staging area of a scatter workgroup holds its slice; the slices cover the scalars
  if (s.cap != s.slice * p.W || (uint64_t)s.slice * s.n_slices < (uint64_t)p.n * p.J || (uint64_t)s.slice1 * s.n_slices1 < (uint64_t)p.n * p.J) return false;
  // msm_accumulate: the lanes cover the entries, two partial slots each
  if (hp.n_chunks * p.chunk < hp.entries || (p.lanes && p.lanes != hp.n_chunks) || (uint64_t)hp.acc_grid * 256 < hp.n_chunks) return false;
  if (hp.ws.partial < 2 * hp.n_chunks * MSM_SLOT_BYTES || hp.long_cap < hp.n_chunks / FIXUP_LONG + 1) return false;
  // the tree: levels 0 .. c - 2 exactly once, each tmp buffer holds every step written to it, the last step writes the result
  uint32_t k = 0;
  for (uint32_t i = 0; i < hp.n_steps; i++) {
    const MsmTreeStep& t = hp.step[i];
    if (t.k != k || t.m < 1 || t.nodes != p.total >> (k + t.m)) return false;
    if (t.kind == MSM_STEP_LEVEL01 ? (k != 0 || t.m != 2) : (t.kind == MSM_STEP_LEVEL ? t.m != 1 : (t.m > PLANES_STEP_LOG || t.lds > MSM_LDS_DEFAULT))) return false;
    k += t.m;
    if ((t.out == MSM_OUT_FINAL) != (k == p.c - 1)) return false;
    if (t.out != MSM_OUT_FINAL && (size_t)t.nodes * (k + 1) > hp.tmp_slots[t.out]) return false;
    if (i && t.out == hp.step[i - 1].out) return false;      // a launch never reads the buffer it writes
  }
  if (hp.n_steps > MSM_MAX_TREE_STEPS || k != p.c - 1) return false;
  if (hp.n_planes > (uint32_t)MSM_MAX_WINDOWS || hp.n_planes != hp.Wr * hp.per_window) return false;
  // the memset stays inside msm.ctl, the run tickets behind the long-bucket tickets
  return hp.run_ticket == 8 + PART_MAX + hp.long_cap && hp.ctl_zeroed == hp.run_ticket + hp.n_final && hp.ctl_zeroed <= hp.ctl_words &&
         hp.ws.ctl == (size_t)hp.ctl_words * 4;
}

}  // namespace bp

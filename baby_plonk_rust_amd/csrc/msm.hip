// msm.hip -- host driver of the G1 MSM pipeline (kernels in msm_kernels.hpp).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ctx.hpp"
#include "msm_kernels.hpp"

namespace bp {

static_assert(sizeof(proj28_slot) == MSM_SLOT_BYTES, "msm_plan.hpp sizes the workspaces by this");

// the only reader of the BP_MSM_* variables (experiment build; the shipped library's knob() answers nullptr, so every default stays).
// The tables of an SRS and the MSMs over them must see the same BP_MSM_RADIX / BP_MSM_RADIX_FROM.
MsmKnobs msm_knobs() { return msm_knobs_read(knob_u32); }

// unsaturated copy of an SRS (128-byte slots) (allocated here, owned by the SRS entry)
int srs_to28_run(bp_ctx* ctx, const g1_affine* d_in, size_t n, g1_affine28** d_out) {
  g1_affine28* d = nullptr;
  BP_HIP(ctx, hipMalloc((void**)&d, (n ? n : 1) * sizeof(g1_affine28)));
  if (n) hipLaunchKernelGGL(srs_to28, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_in, n, d);
  BP_HIP(ctx, hipGetLastError());
  *d_out = d;
  return BP_OK;
}

int srs_to28_into(bp_ctx* ctx, const g1_affine* d_in, size_t n, g1_affine28* d_out) {
  if (n) hipLaunchKernelGGL(srs_to28, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_in, n, d_out);
  BP_HIP(ctx, hipGetLastError());
  return BP_OK;
}

// table[w * n + i] = 2^(c w) P_i (R^w P_i with a radix); row 0 is the unsaturated SRS copy itself
int srs_tables_run(bp_ctx* ctx, const g1_affine* d_points, const g1_affine28* d_points28, size_t n, uint32_t c, g1_affine28** d_table,
                   uint32_t* windows) {
  const uint32_t W = msm_windows(c);
  const MsmRadix* rx = msm_table_radix(c, msm_knobs());
  const uint32_t radix = rx ? rx->R : 0u;             // rows R^w P_i where the MSM cuts radix-R digits (MsmPlan::radix)
  if ((uint64_t)W * n >= (1ull << 31))
    return BP_FAIL(ctx, BP_ERR_TOO_LARGE, "fixed-base tables: windows * points >= 2^31");
  g1_affine28* t = nullptr;
  BP_HIP(ctx, hipMalloc((void**)&t, (size_t)W * (n ? n : 1) * sizeof(g1_affine28)));
  if (n) {
    BP_HIP(ctx, hipMemcpyAsync(t, d_points28, n * sizeof(g1_affine28), hipMemcpyDeviceToDevice, ctx->stream));
    if (radix) hipLaunchKernelGGL(srs_window_tables<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_points28, n, c, W, radix, t);
    else hipLaunchKernelGGL(srs_window_tables<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_points28, n, c, W, 0u, t);
  }
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = stream_wait(ctx->stream);
  if (e != hipSuccess) {
    (void)hipFree(t);
    return fail(ctx, BP_ERR_HIP, "srs_window_tables", e, __FILE__, __LINE__);
  }
  *d_table = t;
  *windows = W;
  return BP_OK;
}

// accumulator slot (lazy 28-bit limbs, as the kernels leave it) -> the reference's Montgomery limbs
static g1_proj slot_to_proj(const proj28_slot* slot) {
  g1_proj28 p;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(slot);
  for (int j = 0; j < N28; j++) { p.x.l[j] = src[j]; p.y.l[j] = src[N28 + j]; p.z.l[j] = src[2 * N28 + j]; }
  return g1_proj_from_28(p);
}

// dynamic-LDS limits are per function AND per device: set them for every context at creation (bp_init), after hipSetDevice
int msm_init_device(bp_ctx* ctx) {
  const struct { const void* kernel; size_t limit; } limits[] = {
      {(const void*)msm_radix_scatter, MSM_LDS_RADIX_SCATTER},
      {(const void*)msm_radix_final<false>, MSM_LDS_RUN_HIST},
      {(const void*)msm_radix_final<true>, MSM_LDS_RUN_HIST},
      {(const void*)msm_radix_long_count<false>, MSM_LDS_RUN_HIST},
      {(const void*)msm_radix_long_count<true>, MSM_LDS_RUN_HIST},
      {(const void*)msm_radix_long_scatter<false>, MSM_LDS_RUN_HIST},
      {(const void*)msm_radix_long_scatter<true>, MSM_LDS_RUN_HIST},
      {(const void*)msm_part_scatter<false, false>, MSM_LDS_PART_SCATTER},
      {(const void*)msm_part_scatter<false, true>, MSM_LDS_PART_SCATTER},
      {(const void*)msm_part_scatter<true, false>, MSM_LDS_PART_SCATTER},
      {(const void*)msm_part_scatter<true, true>, MSM_LDS_PART_SCATTER},
  };
  for (const auto& l : limits) BP_HIP(ctx, hipFuncSetAttribute(l.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.limit));
  return BP_OK;
}

// device buffers of the bucket sort: the workspaces msm.ctl .. msm.run_long (keys / vals: msm.rkeys0 / 1, msm.rvals0 / 1)
struct SortBufs {
  uint32_t *ctl, *counts, *offsets, *cursors, *sorted, *tile_sums, *keys[2], *vals[2], *run_off, *run_cnt, *run_cur, *run_long;
};

// level 1 of either sort (MsmLevel1): 2^pb partitions cut straight from the scalars, their offsets to `off`, their records to keys / vals
static void level1_launch(hipStream_t st, const MsmHostPlan& hp, const MsmScalars& scalars, int fmt, const SortBufs& b, uint32_t* off, uint32_t* keys,
                          uint32_t* vals) {
  const MsmLevel1& s = hp.l1;
  hipLaunchKernelGGL(msm_part_count, dim3(s.n_slices1), dim3(s.count_threads), 0, st, scalars, fmt, hp.dev, s.slice1, s.pb, s.rb, b.ctl + 4, off, b.run_cur, b.ctl + 1);
  const auto scatter = hp.packed ? (hp.flat ? msm_part_scatter<true, true> : msm_part_scatter<true, false>)
                                 : (hp.flat ? msm_part_scatter<false, true> : msm_part_scatter<false, false>);
  hipLaunchKernelGGL(scatter, dim3(s.n_slices), dim3(s.scatter_threads), s.part_lds, st, scalars, fmt, hp.dev, s.slice, s.pb, s.rb, hp.sort == 2 ? hp.vb : 0u, s.cap,
                     b.run_cur, keys, vals);
}

// the final runs of either sort, for one record form: each sorted in one workgroup's histogram, the long runs among them slice-parallel
template <bool PACKED>
static void final_runs_launch(hipStream_t st, const MsmHostPlan& hp, const SortBufs& b, const uint32_t* keys, const uint32_t* vals, const uint32_t* off) {
  const uint32_t total = hp.dev.total;
  uint32_t *rlong_n = b.ctl + 2, *run_ticket = b.ctl + hp.run_ticket;
  const RunRecords<PACKED> rr{keys, vals, (1u << hp.rbits) - 1u, PACKED ? hp.vb : 0u};       // vals: null with packed records
  hipLaunchKernelGGL(msm_radix_final<PACKED>, dim3(hp.final_grid), dim3(hp.final_threads), hp.rhist, st, rr, off, hp.n_final, hp.rbits, total, b.offsets, b.sorted,
                     rlong_n, b.run_long, b.counts);
  if (hp.long_gx) {
    const dim3 lgrid(hp.long_gx, hp.long_gy);
    hipLaunchKernelGGL(msm_radix_long_count<PACKED>, lgrid, dim3(1024), hp.rhist, st, rr, off, hp.n_final, hp.rbits, total, rlong_n, b.run_long, b.counts, b.offsets,
                       b.cursors, run_ticket);
    hipLaunchKernelGGL(msm_radix_long_scatter<PACKED>, lgrid, dim3(1024), hp.rhist, st, rr, off, hp.rbits, rlong_n, b.run_long, b.cursors, b.sorted);
  }
}

// d_points28: the unsaturated SRS copy, or (table_c != 0) row 0 of its fixed-base tables with rows table_stride apart.
// Enqueues the whole pipeline and the device-to-host copy of the window sums on ctx->stream; waits for nothing.
int msm_launch(bp_ctx* ctx, const g1_affine28* d_points28, size_t n, const fr_t* d_scalars, int fmt, uint32_t table_c, size_t table_stride,
               int slot, void* d_blob, MsmPending* out) {
  return msm_launch_many(ctx, d_points28, 1, &d_scalars, &n, fmt, table_c, table_stride, slot, d_blob, out);
}

// J scalar vectors against the same points in one pipeline (J > 1: fixed-base tables only, results in the pinned slot only);
// vector j has n_each[j] scalars.  msm_finish then delivers J results.  Every decision is msm_plan's (msm_plan.hpp): this function
// allocates by the plan's sizes and launches by its fields.
int msm_launch_many(bp_ctx* ctx, const g1_affine28* d_points28, uint32_t J, const fr_t* const* d_scalars_each, const size_t* n_each, int fmt,
                    uint32_t table_c, size_t table_stride, int slot, void* d_blob, MsmPending* out) {
  *out = MsmPending();
  out->blob = d_blob != nullptr;
  const MsmHostPlan hp = msm_plan(J, n_each, table_c, table_stride, d_blob != nullptr, msm_knobs());
  if (hp.err == BP_ERR_INVALID_ARG) return BP_FAIL(ctx, hp.err, hp.what);       // a batch no pipeline takes: refused before anything else
  out->J = J;
  if (hp.empty) {
    if (d_blob) {
      MsmBlobHeader hdr;
      memset(&hdr, 0, sizeof hdr);
      hdr.magic = MSM_BLOB_MAGIC;
      hipLaunchKernelGGL(msm_write_blob, dim3(1), dim3(64), 0, ctx->stream, (const proj28_slot*)nullptr, hdr, (uint8_t*)d_blob);
      BP_HIP(ctx, hipGetLastError());
    }
    return BP_OK;
  }
  if (slot < 0 || slot >= MSM_SLOTS) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "MSM result slot");
  if (hp.err) return BP_FAIL(ctx, hp.err, hp.what);                             // too long, too many windows
  const MsmPlan& plan = hp.dev;
  MsmScalars scalars_all;
  for (uint32_t j = 0; j < MSM_MAX_BATCH; j++) scalars_all.p[j] = j < J ? d_scalars_each[j] : nullptr;
  SortBufs b = {};
  uint32_t* long_list;
  proj28_slot *long_scratch, *bucket_sum, *partial, *roots = nullptr, *window_sum, *tmp[2] = {nullptr, nullptr};
  const struct { const char* name; size_t bytes; void** p; } buffers[] = {
      {"msm.ctl", hp.ws.ctl, (void**)&b.ctl},
      {"msm.counts", hp.ws.counts, (void**)&b.counts},
      {"msm.offsets", hp.ws.offsets, (void**)&b.offsets},
      {"msm.cursors", hp.ws.cursors, (void**)&b.cursors},
      {"msm.long_list", hp.ws.long_list, (void**)&long_list},
      {"msm.long_scratch", hp.ws.long_scratch, (void**)&long_scratch},
      {"msm.tile_sums", hp.ws.tile_sums, (void**)&b.tile_sums},
      {"msm.sorted", hp.ws.sorted, (void**)&b.sorted},
      {"msm.bucket_sum", hp.ws.bucket_sum, (void**)&bucket_sum},
      {"msm.partial", hp.ws.partial, (void**)&partial},
      {"msm.roots", hp.ws.roots, (void**)&roots},
      {"msm.window_sum", hp.ws.window_sum, (void**)&window_sum},
      {"msm.rkeys0", hp.ws.rkeys0, (void**)&b.keys[0]},
      {"msm.rvals0", hp.ws.rvals0, (void**)&b.vals[0]},
      {"msm.rkeys1", hp.ws.rkeys1, (void**)&b.keys[1]},
      {"msm.rvals1", hp.ws.rvals1, (void**)&b.vals[1]},
      {"msm.run_off", hp.ws.run_off, (void**)&b.run_off},
      {"msm.run_cnt", hp.ws.run_cnt, (void**)&b.run_cnt},
      {"msm.run_cur", hp.ws.run_cur, (void**)&b.run_cur},
      {"msm.run_long", hp.ws.run_long, (void**)&b.run_long},
      {"msm.planes_tmp0", hp.ws.planes_tmp0, (void**)&tmp[0]},
      {"msm.planes_tmp1", hp.ws.planes_tmp1, (void**)&tmp[1]},
  };
  for (const auto& w : buffers)
    if (w.bytes) BP_TRY(ws_get(ctx, w.name, w.bytes, w.p));      // 0 bytes: this pipeline does not use it, the pointer stays null
  // pinned staging: MSM_SLOTS result areas of the largest possible size, so earlier pending results stay where they are
  constexpr size_t slot_bytes = (size_t)MSM_MAX_WINDOWS * sizeof(proj28_slot) + 16;
  uint8_t* h_base;
  BP_TRY(pinned_get(ctx, MSM_SLOTS * slot_bytes, (void**)&h_base));
  proj28_slot* h_windows = reinterpret_cast<proj28_slot*>(h_base + (size_t)slot * slot_bytes);
  const uint32_t total = plan.total, n_planes = hp.n_planes;
  uint32_t *offsets = b.offsets, *long_count = b.ctl, *status = b.ctl + 1, *long_ticket = b.ctl + 8 + PART_MAX;      // the control words: MsmHostPlan
  hipStream_t st = ctx->stream;
  BP_HIP(ctx, hipEventRecord(ctx->ev[0], st));
  BP_HIP(ctx, hipMemsetAsync(b.ctl, 0, (size_t)hp.ctl_zeroed * 4, st));
  if (hp.sort == 2) {
    level1_launch(st, hp, scalars_all, fmt, b, b.run_off, b.keys[0], b.vals[0]);
    (hp.packed ? final_runs_launch<true> : final_runs_launch<false>)(st, hp, b, b.keys[0], b.vals[0], b.run_off);
  } else {
    uint32_t* const run_off[2] = {b.run_off + 4,                     // after level 1: 2^lv[0] + 1 entries
                                  b.run_off + 8 + hp.n_final};       // after level 2: n_final + 1 entries
    level1_launch(st, hp, scalars_all, fmt, b, run_off[0], b.keys[1], b.vals[1]);
    uint32_t side = 1;
    if (hp.lv[1]) {                 // the second level: msm_radix_count / _scatter cut each run of level 1 by the next lv[1] bits
      const dim3 grid(hp.gx2, 1u << hp.lv[0]);
      BP_HIP(ctx, hipMemsetAsync(b.run_cnt, 0, (size_t)hp.n_sub * 4, st));
      hipLaunchKernelGGL(msm_radix_count, grid, dim3(1024), 0, st, b.keys[side], run_off[0], hp.shift2, hp.lv[1], b.run_cnt);
      hipLaunchKernelGGL(scan_tile_sums, dim3(hp.scan_tiles), dim3(256), 0, st, b.run_cnt, hp.n_sub, b.tile_sums);
      hipLaunchKernelGGL(scan_block_sums, dim3(1), dim3(256), 0, st, b.tile_sums, hp.scan_tiles, run_off[1] + hp.n_sub);
      hipLaunchKernelGGL(scan_apply, dim3(hp.scan_tiles), dim3(256), 0, st, b.run_cnt, hp.n_sub, b.tile_sums, run_off[1], b.run_cur);
      hipLaunchKernelGGL(msm_radix_scatter, grid, dim3(1024), RADIX_SLICE * 9, st, b.keys[side], b.vals[side], run_off[0], hp.shift2, hp.lv[1], b.run_cur,
                         b.keys[side ^ 1], b.vals[side ^ 1]);
      side ^= 1;
    }
    final_runs_launch<false>(st, hp, b, b.keys[side], b.vals[side], run_off[hp.lv[1] ? 1 : 0]);
  }
  BP_HIP(ctx, hipEventRecord(ctx->ev[1], st));
  hipLaunchKernelGGL(msm_accumulate<2>, dim3(hp.acc_grid), dim3(256), 0, st, d_points28, b.sorted, offsets, plan, bucket_sum, partial);
  BP_HIP(ctx, hipEventRecord(ctx->ev[2], st));
  if (hp.by_edges)
    hipLaunchKernelGGL(msm_fixup_edges, dim3(hp.fixup_grid), dim3(256), 0, st, offsets, plan, bucket_sum, partial, long_count, long_list, hp.long_cap);
  else if (table_c)
    hipLaunchKernelGGL(msm_fixup<2>, dim3(hp.fixup_grid), dim3(256), 0, st, offsets, plan, bucket_sum, partial, long_count, long_list, hp.long_cap);
  else
    hipLaunchKernelGGL(msm_fixup<1>, dim3(hp.fixup_grid), dim3(256), 0, st, offsets, plan, bucket_sum, partial, long_count, long_list, hp.long_cap);
  hipLaunchKernelGGL(msm_fixup_long, dim3(512), dim3(256), 256 * sizeof(proj28_slot), st, offsets, plan, bucket_sum, partial, long_count, long_list, hp.long_cap,
                     long_scratch, long_ticket);
  // the bucket tree, launch by launch; the last one writes where the epilogue reads (tables: the window sums and the status word behind them)
  uint32_t* const status_out = reinterpret_cast<uint32_t*>(window_sum + n_planes);
  const proj28_slot* in = bucket_sum;
  for (uint32_t i = 0; i < hp.n_steps; i++) {
    const MsmTreeStep& s = hp.step[i];
    const bool last = s.out == MSM_OUT_FINAL;
    proj28_slot* out_nodes = last ? (table_c ? window_sum : roots) : tmp[s.out];
    const dim3 grid(s.gx, s.gy);
    if (s.kind == MSM_STEP_LEVEL01) {
      hipLaunchKernelGGL(msm_planes_level01, grid, dim3(256), 0, st, offsets, in, s.nodes, out_nodes);
    } else if (s.kind == MSM_STEP_LEVEL) {
      hipLaunchKernelGGL(msm_planes_level, grid, dim3(256), 0, st, offsets, in, s.k, s.nodes, out_nodes);
    } else {
      uint32_t* so = last && table_c ? status_out : (uint32_t*)nullptr;
      if (s.k == 0) hipLaunchKernelGGL(msm_planes_step<true>, grid, dim3(256), s.lds, st, offsets, in, s.k, s.m, out_nodes, status, offsets + total, so);
      else hipLaunchKernelGGL(msm_planes_step<false>, grid, dim3(256), s.lds, st, offsets, in, s.k, s.m, out_nodes, status, offsets + total, so);
    }
    in = out_nodes;
  }
  if (!table_c)           // W roots of c values each -> W x quads partial Horner values (the host finishes what msm.rs:42-46, 107-115 compute)
    hipLaunchKernelGGL(msm_planes_window_quads, dim3(plan.W), dim3(64), 0, st, roots, plan.c, hp.quads, window_sum, status, offsets + total, status_out);
  BP_HIP(ctx, hipGetLastError());
  if (d_blob) {
    MsmBlobHeader hdr;
    memset(&hdr, 0, sizeof hdr);
    hdr.magic = MSM_BLOB_MAGIC;
    hdr.c = plan.c;
    hdr.Wr = table_c ? 1 : hp.Wr;
    hdr.n_planes = n_planes;
    hdr.tables = table_c != 0;
    hdr.quads = table_c ? 0u : hp.quads;
    hipLaunchKernelGGL(msm_write_blob, dim3(1), dim3(256), 0, st, window_sum, hdr, (uint8_t*)d_blob);
    BP_HIP(ctx, hipGetLastError());
  } else {
    BP_HIP(ctx, hipMemcpyAsync(h_windows, window_sum, (size_t)n_planes * sizeof(proj28_slot) + 8, hipMemcpyDeviceToHost, st));    // sums + status + entry count
  }
  BP_HIP(ctx, hipEventRecord(ctx->ev[3], st));
  out->empty = false;
  out->tables = table_c != 0;
  out->c = plan.c;
  out->Wr = table_c ? 1 : hp.Wr;
  out->n_planes = n_planes;
  out->quads = hp.quads;
  out->adds = hp.entries;       // upper bound (blob mode keeps it); msm_finish replaces it by the exact count of non-zero digits
  out->h_windows = h_windows;
  msm_plan_path(hp, ctx->msm_path);      // what this launch decided (bp_msm_last_path): host words only, set once everything is enqueued
  return BP_OK;
}

// ---- host epilogue: Horner over what the device hands over
// quads[w * nq + j] = the part of window w's sum that carries the factor 2^(4j) (msm_planes_window_quads):
//   out = sum_w 2^(c w) sum_j 2^(4 j) quads[w][j], one Horner pass from the top position down -- c (W - 1) + 4 (nq - 1) doublings, the same
//   dependent chain the W window sums needed (nq = 1: one value per window, the reference's combine, msm.rs:107-115)
static void host_quad_horner(g1_proj& out, const g1_proj* quads, uint32_t W, uint32_t c, uint32_t nq) {
  g1_proj acc = g1_identity();
  uint32_t prev = 0;
  bool first = true;
  for (uint32_t w = W; w-- > 0;)
    for (uint32_t j = nq; j-- > 0;) {
      const uint32_t pos = c * w + 4 * j;
      if (first) {
        acc = quads[(size_t)w * nq + j];
        first = false;
      } else {
        for (uint32_t d = pos; d < prev; d++) g1_double(acc, acc);
        g1_add(acc, acc, quads[(size_t)w * nq + j]);
      }
      prev = pos;
    }
  out = acc;
}

// planes[w * c + 0] = A_w, planes[w * c + 1 + j] = T_{w,j} (j < c - 1):
//   out = sum_w 2^(c w) (A_w + sum_j 2^j T_{w,j}),  one pass from the top bit position down (bucket b holds digit b + 1)
static void host_plane_horner(g1_proj& out, const g1_proj* planes, uint32_t W, uint32_t c) {
  g1_proj acc = g1_identity();
  for (uint32_t w = W; w-- > 0;) {
    const g1_proj* p = planes + (size_t)w * c;
    for (uint32_t j = c; j-- > 0;) {
      g1_double(acc, acc);
      if (j + 1 < c) g1_add(acc, acc, p[1 + j]);           // bit position c - 1 of the window carries no plane
    }
    g1_add(acc, acc, p[0]);
  }
  out = acc;
}

// waits for the stream, checks the scalar status and runs the host epilogue: window sums / planes back to the reference's
// Montgomery limbs, then Horner (msm.rs:107-115).  The timing stats describe the last launched MSM of this ctx.
int msm_finish(bp_ctx* ctx, const MsmPending& pend, g1_proj* host_out) {
  ctx->msm_async_pending = false;
  if (pend.empty) {
    for (uint32_t j = 0; host_out && j < pend.J; j++) host_out[j] = g1_identity();
    ctx->msm_accumulate_ms = ctx->msm_total_ms = 0;
    ctx->msm_adds = 0;
    if (pend.blob) BP_HIP(ctx, stream_wait(ctx->stream));
    return BP_OK;
  }
  BP_HIP(ctx, stream_wait(ctx->stream));
  BP_HIP(ctx, hipEventElapsedTime(&ctx->msm_accumulate_ms, ctx->ev[1], ctx->ev[2]));
  BP_HIP(ctx, hipEventElapsedTime(&ctx->msm_total_ms, ctx->ev[0], ctx->ev[3]));
  ctx->msm_c = pend.c;
  ctx->msm_tables = pend.tables;
  ctx->msm_adds = pend.adds;
  if (pend.blob) {                      // the result stayed in HBM (bp_msm_g1_blob_device); its status word travels in the record
    if (host_out) *host_out = g1_identity();
    return BP_OK;
  }
  const proj28_slot* h_windows = static_cast<const proj28_slot*>(pend.h_windows);
  const uint32_t n_planes = pend.n_planes;
  const uint32_t* tail = reinterpret_cast<const uint32_t*>(h_windows + n_planes);
  if (tail[0]) return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, "scalar >= q in a canonical-bytes input");
  ctx->msm_adds = tail[1];             // entries of the bucket-sorted list = non-zero digits = bucket additions performed
  std::vector<g1_proj> windows(n_planes);
  for (uint32_t w = 0; w < n_planes; w++) windows[w] = slot_to_proj(&h_windows[w]);
  if (pend.tables) {
    for (uint32_t j = 0; j < pend.J; j++)              // a batch: c values per vector, one Horner pass each
      host_plane_horner(host_out[j], windows.data() + (size_t)j * pend.c, pend.Wr, pend.c);
  } else {
    host_quad_horner(*host_out, windows.data(), pend.Wr, pend.c, pend.quads);
  }
  return BP_OK;
}

// Host side of the one-process-per-GPU exchange: n_blobs records (BP_MSM_BLOB_BYTES apart, host memory).  Records that
// share the window layout (the normal case: equal shard sizes) are added slot by slot first, so the Horner pass over the
// c bit positions (msm.rs:107-115) runs once instead of once per rank.
int msm_blobs_combine(const uint8_t* blobs, size_t n_blobs, g1_proj* out) {
  g1_proj total = g1_identity();
  std::vector<bool> done(n_blobs, false);
  for (size_t i = 0; i < n_blobs; i++) {
    MsmBlobHeader h;
    memcpy(&h, blobs + i * BP_MSM_BLOB_BYTES, sizeof h);
    if (h.magic != MSM_BLOB_MAGIC || h.n_planes > (uint32_t)MSM_MAX_WINDOWS) return BP_ERR_INVALID_ARG;
    if (h.err != 0) return h.err < 0 && h.err >= BP_ERR_COMM ? h.err : BP_ERR_INVALID_ARG;       // a rank's poisoned record: its code for every rank (msm_blob_poisoned names the rank)
    // the Horner passes below index the slots by (Wr, c): a record whose header does not describe its own slot count (another
    // library version on a peer rank, a truncated gather) is rejected here instead of being read past its end
    if (h.tables > 1) return BP_ERR_INVALID_ARG;          // 0 or 1; any other value is another library's record (older experiment builds wrote 2)
    if (h.n_planes != 0) {
      const bool width_ok = h.c >= 2 && h.c <= (uint32_t)MSM_MAX_TABLE_C;
      const uint32_t per = h.tables ? h.c : (h.quads ? h.quads : 1u);
      if (!width_ok || h.Wr < 1 || per > 8 * 4 || h.n_planes != h.Wr * per) return BP_ERR_INVALID_ARG;
    }
    if (h.status) return BP_ERR_BAD_SCALAR;
  }
  for (size_t i = 0; i < n_blobs; i++) {
    if (done[i]) continue;
    MsmBlobHeader h;
    memcpy(&h, blobs + i * BP_MSM_BLOB_BYTES, sizeof h);
    done[i] = true;
    if (h.n_planes == 0) continue;
    std::vector<g1_proj> sum(h.n_planes);
    const proj28_slot* slots = reinterpret_cast<const proj28_slot*>(blobs + i * BP_MSM_BLOB_BYTES + sizeof(MsmBlobHeader));
    for (uint32_t w = 0; w < h.n_planes; w++) sum[w] = slot_to_proj(&slots[w]);
    for (size_t k = i + 1; k < n_blobs; k++) {
      MsmBlobHeader g;
      memcpy(&g, blobs + k * BP_MSM_BLOB_BYTES, sizeof g);
      if (done[k] || g.c != h.c || g.Wr != h.Wr || g.n_planes != h.n_planes || g.tables != h.tables || g.quads != h.quads) continue;
      done[k] = true;
      const proj28_slot* sk = reinterpret_cast<const proj28_slot*>(blobs + k * BP_MSM_BLOB_BYTES + sizeof(MsmBlobHeader));
      for (uint32_t w = 0; w < h.n_planes; w++) g1_add(sum[w], sum[w], slot_to_proj(&sk[w]));
    }
    g1_proj part;
    if (h.tables) host_plane_horner(part, sum.data(), h.Wr, h.c);
    else host_quad_horner(part, sum.data(), h.Wr, h.c, h.quads ? h.quads : 1u);
    g1_add(total, total, part);
  }
  *out = total;
  return BP_OK;
}

// first poisoned record among n_blobs host records: its error code (0: none) and the rank that wrote it
int msm_blob_poisoned(const uint8_t* blobs, size_t n_blobs, uint32_t* rank) {
  for (size_t i = 0; i < n_blobs; i++) {
    MsmBlobHeader h;
    memcpy(&h, blobs + i * BP_MSM_BLOB_BYTES, sizeof h);
    if (h.magic == MSM_BLOB_MAGIC && h.err != 0) {
      if (rank) *rank = h.err_rank;
      return h.err < 0 && h.err >= BP_ERR_COMM ? h.err : BP_ERR_INVALID_ARG;
    }
  }
  return 0;
}

// this rank's record when its MSM failed before the collective: header only, on the context's stream
int msm_blob_poison_run(bp_ctx* ctx, void* d_blob, int err, uint32_t rank) {
  MsmBlobHeader hdr;
  memset(&hdr, 0, sizeof hdr);
  hdr.magic = MSM_BLOB_MAGIC;
  hdr.err = err;
  hdr.err_rank = rank;
  hipLaunchKernelGGL(msm_write_blob, dim3(1), dim3(64), 0, ctx->stream, (const proj28_slot*)nullptr, hdr, (uint8_t*)d_blob);
  BP_HIP(ctx, hipGetLastError());
  return BP_OK;
}

int msm_blobs_sum_device_run(bp_ctx* ctx, const void* d_blobs, size_t n_blobs, void* d_out, bool wait) {
  hipLaunchKernelGGL(msm_blob_sum, dim3((MSM_MAX_WINDOWS + 7) / 8), dim3(64), 0, ctx->stream, (const uint8_t*)d_blobs, (uint32_t)n_blobs,
                     (uint32_t)BP_MSM_BLOB_BYTES, (uint8_t*)d_out);
  BP_HIP(ctx, hipGetLastError());
  if (wait) BP_HIP(ctx, stream_wait(ctx->stream));
  return BP_OK;
}

int msm_run(bp_ctx* ctx, const g1_affine28* d_points28, size_t n, const fr_t* d_scalars, int fmt, uint32_t table_c, size_t table_stride,
            g1_proj* host_out) {
  MsmPending pend;
  BP_TRY(msm_launch(ctx, d_points28, n, d_scalars, fmt, table_c, table_stride, 0, nullptr, &pend));
  return msm_finish(ctx, pend, host_out);
}

}  // namespace bp

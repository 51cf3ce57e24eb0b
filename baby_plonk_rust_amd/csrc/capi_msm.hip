// capi_msm.hip -- C ABI, part 2b: the G1 MSM entry points (BucketMSM::bucket_msm, Setup::commit over one GPU or the shards of a
// group context, commit lanes, records for the one-process-per-GPU path) and their stats.  The SRS they read lives in capi_srs.hip.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ctx.hpp"

#include "capi_common.hpp"

using namespace bp;

// Enqueue the MSM of one shard: scalars[0..n) against the member's points [local_first, local_first + n).
//   where 0: `scalars` is host memory; 1: HBM of this member's device; 2: HBM of device src_device (the leader's): copied
//   GPU to GPU into the member's workspace once the leader's stream has reached `ready`.
static int msm_shard_launch(bp_ctx* m, SrsEntry* e, size_t local_first, const void* scalars, size_t n, int fmt, int where, int src_device,
                            hipEvent_t ready, int slot, void* d_blob, MsmPending* pend) {
  DeviceGuard guard(m->device);
  const fr_t* d_scalars = (const fr_t*)scalars;
  if (where != 1 && n) {
    fr_t* d;
    BP_TRY(ws_get(m, "io.scalars", n * sizeof(fr_t), (void**)&d));
    if (where == 0) {
      BP_HIP(m, hipEventRecord(m->ev[4], m->stream));            // upload = ev[4] .. ev[0] (msm_launch records ev[0] first thing)
      BP_HIP(m, hipMemcpyAsync(d, scalars, n * sizeof(fr_t), hipMemcpyHostToDevice, m->stream));
    } else {
      BP_HIP(m, hipStreamWaitEvent(m->stream, ready, 0));
      if (!peer_path(m, src_device)) BP_HIP(m, hipMemcpyAsync(d, scalars, n * sizeof(fr_t), hipMemcpyDeviceToDevice, m->stream));
      else BP_HIP(m, hipMemcpyPeerAsync(d, m->device, scalars, src_device, n * sizeof(fr_t), m->stream));
    }
    d_scalars = d;
  }
  if (srs_tables_pay(*e, n)) return msm_launch(m, e->d_table + local_first, n, d_scalars, fmt, e->table_c, e->n, slot, d_blob, pend);
  return msm_launch(m, e->d_points28 + local_first, n, d_scalars, fmt, 0, 0, slot, d_blob, pend);
}

// sum_{i < n} s_i P_{first + i} over every shard of the SRS, in two steps so that several such sums can be in flight:
// launch enqueues every shard's whole pipeline (result slot `slot` of each member), finish waits and adds the partial sums.
struct ShardedPending {
  std::vector<MsmPending> pend;
  std::vector<bool> used;
  bool host_scalars = false;
};
static int msm_all_shards_launch(bp_ctx* ctx, uint64_t srs_handle, size_t first, const void* scalars, size_t n_scalars, int scalar_fmt,
                                 int scalars_on_device, int slot, ShardedPending* sp) {
  std::vector<SrsShard> sh;
  BP_TRY(srs_shards(ctx, srs_handle, &sh, first, n_scalars));            // more scalars than points: cut to the SRS (zip() truncation, msm.rs:29)
  if (first > sh[0].e->n_global) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "SRS offset out of bounds");
  if (sh.size() > 1 && scalars_on_device) {            // the members' copies must see what the leader's stream has produced
    DeviceGuard guard(ctx->device);
    BP_HIP(ctx, hipEventRecord(ctx->ev[4], ctx->stream));
  }
  sp->pend.assign(sh.size(), MsmPending());
  sp->used.assign(sh.size(), false);
  sp->host_scalars = !scalars_on_device;
  // the launches: scalars already in HBM are enqueued by this thread (asynchronous copies and kernels);
  // host scalars go through the members' own threads, so that the uploads -- staged by the issuing thread when the memory is
  // pageable, as a Rust Vec<Scalar> is -- run on all PCIe links at once instead of one after another
  std::vector<int> rcs(sh.size(), BP_OK);
  std::vector<bool> take(sh.size(), false);
  // a shard none of the range lies on is skipped -- except the only shard of a plain context: the empty MSM resets the stats and yields the identity
  for (size_t r = 0; r < sh.size(); r++) take[r] = sh[r].lo < sh[r].hi || sh.size() == 1;
  auto launch_one = [&](size_t r) {
    const SrsShard& s = sh[r];
    const bool any = s.lo < s.hi;
    const int where = !scalars_on_device ? 0 : (r == 0 ? 1 : 2);
    rcs[r] = msm_shard_launch(s.m, s.e, any ? s.lo - s.e->first : 0, (const uint8_t*)scalars + (any ? (s.lo - first) * sizeof(fr_t) : 0), any ? s.hi - s.lo : 0,
                              scalar_fmt, where, ctx->device, ctx->ev[4], slot, nullptr, &sp->pend[r]);
  };
  if (!scalars_on_device && sh.size() > 1) {
    over_members(ctx, sh.size(), [&](size_t r) { return (bool)take[r]; }, launch_one);
  } else {
    for (size_t r = 0; r < sh.size(); r++)
      if (take[r]) launch_one(r);
  }
  int rc = BP_OK;
  for (size_t r = 0; r < sh.size(); r++) {
    if (!take[r]) continue;
    sp->used[r] = rcs[r] == BP_OK;             // a shard that failed to launch has nothing to wait for
    const int rc1 = lift(ctx, sh[r].m, rcs[r]);
    if (rc == BP_OK) rc = rc1;
  }
  return rc;               // the caller still finishes whatever was launched
}
static int msm_all_shards_finish(bp_ctx* ctx, const ShardedPending& sp, int rc, g1_proj* out) {
  const std::vector<bp_ctx*> sh = shards_of(ctx);
  const std::vector<MsmPending>& pend = sp.pend;
  const std::vector<bool>& used = sp.used;
  if (pend.size() != sh.size()) return rc != BP_OK ? rc : BP_ERR_INVALID_ARG;      // nothing was launched (bad handle / offset)
  // every launched shard is waited for, also after a failure elsewhere.  In a group the waits and the host epilogues (window
  // sums -> Horner, ~0.1 ms each) run on the members' own threads: eight in sequence would cost more than the shards' GPU time
  // of a 2^20-point MSM split eight ways.
  std::vector<g1_proj> part(sh.size());
  std::vector<int> rcs(sh.size(), BP_OK);
  over_members(ctx, sh.size(), [&](size_t r) { return (bool)used[r]; }, [&](size_t r) {
    DeviceGuard guard(sh[r]->device);
    rcs[r] = msm_finish(sh[r], pend[r], &part[r]);
    sh[r]->shard_accumulate_ms = sh[r]->msm_accumulate_ms;
    sh[r]->shard_total_ms = sh[r]->msm_total_ms;
    sh[r]->shard_adds = sh[r]->msm_adds;
    sh[r]->msm_upload_ms = 0;
    if (rcs[r] == BP_OK && sp.host_scalars && !pend[r].empty && hipEventElapsedTime(&sh[r]->msm_upload_ms, sh[r]->ev[4], sh[r]->ev[0]) != hipSuccess) {
      (void)hipGetLastError();
      sh[r]->msm_upload_ms = 0;
    }
  });
  g1_proj acc = g1_identity();
  float acc_ms = 0, dev_ms = 0;
  uint64_t adds = 0;
  for (size_t r = 0; r < sh.size(); r++) {
    if (!used[r]) continue;
    const int rc1 = lift(ctx, sh[r], rcs[r]);
    if (rc1 != BP_OK) {
      if (rc == BP_OK) rc = rc1;
      continue;
    }
    if (sh.size() == 1) acc = part[r]; else g1_add(acc, acc, part[r]);
    acc_ms = std::max(acc_ms, sh[r]->msm_accumulate_ms);
    dev_ms = std::max(dev_ms, sh[r]->msm_total_ms);
    adds += sh[r]->msm_adds;
  }
  if (rc != BP_OK) return rc;
  if (sh.size() > 1) {                                   // stats of a group: the slowest shard, all additions
    ctx->msm_accumulate_ms = acc_ms;
    ctx->msm_total_ms = dev_ms;
    ctx->msm_adds = adds;
  }
  *out = acc;
  return BP_OK;
}
static int msm_all_shards(bp_ctx* ctx, uint64_t srs_handle, size_t first, const void* scalars, size_t n_scalars, int scalar_fmt,
                          int scalars_on_device, g1_proj* out) {
  ShardedPending sp;
  const int rc = msm_all_shards_launch(ctx, srs_handle, first, scalars, n_scalars, scalar_fmt, scalars_on_device, 0, &sp);
  return msm_all_shards_finish(ctx, sp, rc, out);
}


namespace bp {
constexpr int MAX_LANES = 3;

// k commitments of HBM-resident coefficient vectors (on the leader) over the members of a group: per batch of up to MSM_MAX_BATCH
// vectors every member receives its slice of each (peer copies behind the leader's event), runs ONE pipeline over the slices'
// bucket sets and delivers one partial sum per vector; the host adds the members' partial sums.  BP_ERR_TOO_LARGE before anything
// was launched = a member's batch does not fit one pipeline.
static int commit_many_group_batched(bp_ctx* ctx, uint64_t srs_handle, const fr_t* const* d_coeffs, const size_t* n, int k, g1_proj* out) {
  std::vector<SrsShard> sh;
  BP_TRY(srs_shards(ctx, srs_handle, &sh));
  const size_t R = sh.size(), n_global = sh[0].e->n_global;
  for (const SrsShard& s : sh)
    if (!s.e->d_table) return BP_ERR_TOO_LARGE;
  for (int base = 0; base < k; base += MSM_MAX_BATCH) {
    const int cnt = std::min((int)MSM_MAX_BATCH, k - base);
    {
      DeviceGuard guard(ctx->device);
      BP_HIP(ctx, hipEventRecord(ctx->ev[4], ctx->stream));          // the coefficient vectors were produced on the leader's stream
    }
    std::vector<MsmPending> pend(R);
    std::vector<int> rcs(R, BP_OK);
    std::vector<bool> used(R, false);
    int rc = BP_OK;
    for (size_t r = 0; r < R && rc == BP_OK; r++) {
      bp_ctx* m = sh[r].m;
      const SrsEntry* e = sh[r].e;
      DeviceGuard guard(m->device);
      const fr_t* ptrs[MSM_MAX_BATCH];
      size_t lens[MSM_MAX_BATCH], total = 0;
      for (int j = 0; j < cnt; j++) {
        const size_t nj = std::min(n[base + j], n_global);              // zip() truncation, msm.rs:29
        lens[j] = nj > e->first ? std::min(nj - e->first, e->n) : 0;
        total += lens[j];
      }
      if (total == 0) continue;
      if (r == 0) {
        for (int j = 0; j < cnt; j++) ptrs[j] = d_coeffs[base + j] + e->first;
      } else {
        fr_t* d;
        rc = lift(ctx, m, ws_get(m, "io.scalars", total * sizeof(fr_t), (void**)&d));
        if (rc != BP_OK) break;
        hipError_t he = hipStreamWaitEvent(m->stream, ctx->ev[4], 0);
        size_t at = 0;
        for (int j = 0; j < cnt && he == hipSuccess; j++) {
          if (lens[j]) {
            const fr_t* src = d_coeffs[base + j] + e->first;
            if (!peer_path(m, ctx->device)) he = hipMemcpyAsync(d + at, src, lens[j] * sizeof(fr_t), hipMemcpyDeviceToDevice, m->stream);
            else he = hipMemcpyPeerAsync(d + at, m->device, src, ctx->device, lens[j] * sizeof(fr_t), m->stream);
          }
          ptrs[j] = d + at;
          at += lens[j];
        }
        if (he != hipSuccess) { rc = fail(ctx, BP_ERR_HIP, "commit batch: scalar slices", he, __FILE__, __LINE__); break; }
      }
      // (the tables are used whatever the slice lengths: skipping them for very short slices is a speed heuristic of the single path)
      rcs[r] = msm_launch_many(m, e->d_table, (uint32_t)cnt, ptrs, lens, BP_FR_MONT, e->table_c, e->n, 0, nullptr, &pend[r]);
      if (rcs[r] == BP_ERR_TOO_LARGE && r == 0 && base == 0) return BP_ERR_TOO_LARGE;
      used[r] = rcs[r] == BP_OK;
      rc = lift(ctx, m, rcs[r]);
    }
    std::vector<g1_proj> part(R * MSM_MAX_BATCH);
    over_members(ctx, R, [&](size_t r) { return (bool)used[r]; }, [&](size_t r) {
      DeviceGuard guard(sh[r].m->device);
      rcs[r] = msm_finish(sh[r].m, pend[r], &part[r * MSM_MAX_BATCH]);
    });
    for (size_t r = 0; r < R; r++)
      if (used[r] && rc == BP_OK) rc = lift(ctx, sh[r].m, rcs[r]);
    if (rc != BP_OK) return rc;
    for (int j = 0; j < cnt; j++) {
      g1_proj acc = g1_identity();
      for (size_t r = 0; r < R; r++)
        if (used[r]) g1_add(acc, acc, part[r * MSM_MAX_BATCH + j]);
      out[base + j] = acc;
    }
  }
  return BP_OK;
}

// lane j of a single-device context: 0 is the context itself, j >= 1 a context of its own on the same device (own stream and
// workspaces).  lane_get creates the lanes up to j that do not exist yet.
static bp_ctx* lane_of(bp_ctx* ctx, int j) { return j == 0 ? ctx : ctx->lanes[j - 1]; }
static int lane_get(bp_ctx* ctx, int j, bp_ctx** out) {
  while ((int)ctx->lanes.size() < j) {
    bp_ctx* lane = nullptr;
    int rc = ctx_create(&lane, ctx->device);
    if (rc != BP_OK) return BP_FAIL(ctx, rc, "commit lane");
    ctx->lanes.push_back(lane);
  }
  *out = lane_of(ctx, j);
  return BP_OK;
}

int commit_many(bp_ctx* ctx, uint64_t srs_handle, const fr_t* const* d_coeffs, const size_t* n, int k, g1_proj* out) {
  if (k <= 0) return BP_OK;
  SrsEntry* e;
  BP_TRY(srs_find(ctx, srs_handle, &e));
  if (is_group(ctx) && k > 1 && e->d_table) {   // group: ONE pipeline per member over its slices of up to MSM_MAX_BATCH commitments
    const char* v = knob("BP_COMMIT_BATCH");
    if (!(v && *v == '0')) {
      int rc = commit_many_group_batched(ctx, srs_handle, d_coeffs, n, k, out);
      if (rc != BP_ERR_TOO_LARGE) return rc;       // too long for one pipeline somewhere: queue the commitments one by one below
    }
  }
  if (is_group(ctx) || k == 1) {            // group: every member queues its shards of up to MSM_SLOTS commitments back to back
    for (int base = 0; base < k; base += MSM_SLOTS) {
      const int cnt = std::min((int)MSM_SLOTS, k - base);
      ShardedPending sp[MSM_SLOTS];
      int rcs[MSM_SLOTS], rc = BP_OK;
      for (int j = 0; j < cnt; j++) rcs[j] = rc == BP_OK ? (rc = msm_all_shards_launch(ctx, srs_handle, 0, d_coeffs[base + j], n[base + j], BP_FR_MONT, 1, j, &sp[j])) : BP_OK;
      for (int j = 0; j < cnt; j++) {
        if (sp[j].pend.empty()) continue;
        const int rc1 = msm_all_shards_finish(ctx, sp[j], rcs[j], &out[base + j]);
        if (rc == BP_OK) rc = rc1;
      }
      if (rc != BP_OK) return rc;
    }
    return BP_OK;
  }
  DeviceGuard guard(ctx->device);
  // One pipeline over the bucket sets of up to MSM_MAX_BATCH commitments (msm_launch_many): one sort keyed (polynomial, bucket),
  // one accumulation, one fix-up, one tree over J x 2^(c-1) buckets -- the latency-bound tail is paid once per round instead of
  // once per commitment.  Needs the SRS's fixed-base tables and a batch short enough for the partition sort.  On ONE device the
  // concurrent lanes below already hide the tails of two commitments under the accumulation of the third, and the batch's
  // three-fold sort is exposed: measured 35.6 ms per 2^20-gate proof against 34.4-35.4 with lanes (profiles/r03_commit_batch_ab.txt),
  // so the batch runs only on request there (BP_COMMIT_BATCH=1).  The members of a group context, whose shards are short and whose
  // pipelines share one stream each, use it by default (above).
  {
    const char* v = knob("BP_COMMIT_BATCH");
    size_t n_max = 0;
    for (int j = 0; j < k; j++) n_max = std::max(n_max, std::min(n[j], e->n));
    if (srs_tables_pay(*e, n_max) && v && *v == '1') {
      bool ok = true;
      for (int base = 0; base < k && ok; base += (int)MSM_MAX_BATCH) {
        const int cnt = std::min((int)MSM_MAX_BATCH, k - base);
        const fr_t* ptrs[MSM_MAX_BATCH];
        size_t lens[MSM_MAX_BATCH];
        for (int j = 0; j < cnt; j++) {
          ptrs[j] = d_coeffs[base + j];
          lens[j] = std::min(n[base + j], e->n);                        // zip() truncation, msm.rs:29
        }
        MsmPending pend;
        int rc = msm_launch_many(ctx, e->d_table, (uint32_t)cnt, ptrs, lens, BP_FR_MONT, e->table_c, e->n, 0, nullptr, &pend);
        if (rc == BP_ERR_TOO_LARGE && base == 0) {                      // too long for one pipeline: the lanes below
          ok = false;
          break;
        }
        if (rc != BP_OK) return rc;
        BP_TRY(msm_finish(ctx, pend, &out[base]));
      }
      if (ok) return BP_OK;
    }
  }
  bp_ctx* last;
  BP_TRY(lane_get(ctx, std::min(MAX_LANES, k) - 1, &last));          // every lane the rounds below use exists before the first launch
  for (int base = 0; base < k; base += MAX_LANES) {
    const int cnt = std::min(MAX_LANES, k - base);
    BP_HIP(ctx, hipEventRecord(ctx->ev[4], ctx->stream));          // the coefficient vectors were produced on ctx->stream
    MsmPending pend[MAX_LANES];
    bool used[MAX_LANES] = {false, false, false};
    int rc = BP_OK;
    for (int j = 0; j < cnt && rc == BP_OK; j++) {
      bp_ctx* lane = lane_of(ctx, j);
      if (lane != ctx) {
        hipError_t he = hipStreamWaitEvent(lane->stream, ctx->ev[4], 0);
        if (he != hipSuccess) { rc = fail(ctx, BP_ERR_HIP, "commit lane wait", he, __FILE__, __LINE__); break; }
      }
      const size_t cnt_j = std::min(n[base + j], e->n);              // zip() truncation, msm.rs:29
      rc = lift(ctx, lane, msm_shard_launch(lane, e, 0, d_coeffs[base + j], cnt_j, BP_FR_MONT, 1, ctx->device, nullptr, 0, nullptr, &pend[j]));
      used[j] = rc == BP_OK;
    }
    for (int j = 0; j < cnt; j++) {                                 // every launched lane is waited for, also after a failure elsewhere
      if (!used[j]) continue;
      bp_ctx* lane = lane_of(ctx, j);
      const int rc1 = lift(ctx, lane, msm_finish(lane, pend[j], &out[base + j]));
      if (rc == BP_OK) rc = rc1;
      if (lane != ctx && rc1 == BP_OK && lane->msm_accumulate_ms > ctx->msm_accumulate_ms) ctx->msm_accumulate_ms = lane->msm_accumulate_ms;
    }
    if (rc != BP_OK) return rc;
  }
  return BP_OK;
}

int commit_lane_launch(bp_ctx* ctx, int j, uint64_t srs_handle, const fr_t* d_coeffs, size_t n, hipEvent_t ready, MsmPending* pend) {
  *pend = MsmPending();
  if (j < 0 || j >= MAX_LANES || is_group(ctx)) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "commit lane");
  SrsEntry* e;
  BP_TRY(srs_find(ctx, srs_handle, &e));
  DeviceGuard guard(ctx->device);
  bp_ctx* lane;
  BP_TRY(lane_get(ctx, j, &lane));
  BP_HIP(ctx, hipStreamWaitEvent(lane->stream, ready, 0));
  return lift(ctx, lane, msm_shard_launch(lane, e, 0, d_coeffs, std::min(n, e->n), BP_FR_MONT, 1, ctx->device, nullptr, 0, nullptr, pend));     // zip() truncation, msm.rs:29
}
int commit_lane_finish(bp_ctx* ctx, int j, const MsmPending& pend, g1_proj* out) {
  bp_ctx* lane = lane_of(ctx, j);
  return lift(ctx, lane, msm_finish(lane, pend, out));
}
}  // namespace bp


int bp_msm_g1_partial(bp_ctx* ctx, uint64_t srs_handle, size_t first, const void* scalars, size_t n_scalars, int scalar_fmt,
                      int scalars_on_device, uint8_t out144[144]) {
  if (!ctx || !out144 || !fmt_ok(scalar_fmt) || (n_scalars && !scalars)) return BP_ERR_INVALID_ARG;
  g1_proj r;
  BP_TRY(msm_all_shards(ctx, srs_handle, first, scalars, n_scalars, scalar_fmt, scalars_on_device, &r));
  memcpy(out144, &r, 144);
  return BP_OK;
}

int bp_msm_g1(bp_ctx* ctx, uint64_t srs_handle, const void* scalars, size_t n_scalars, int scalar_fmt, uint8_t out96[96]) {
  if (!out96) return BP_ERR_INVALID_ARG;
  uint8_t part[144];
  BP_TRY(bp_msm_g1_partial(ctx, srs_handle, 0, scalars, n_scalars, scalar_fmt, 0, part));
  g1_proj r;
  memcpy(&r, part, 144);
  host_encode96(out96, r);
  return BP_OK;
}

// BucketMSM::bucket_msm(points: &[G1Projective], scalars: &[Scalar], ..) (src/msm.rs:76-81) with nothing cached.  From 2^17 pairs the
// operands cross PCIe in pieces on the side context's stream (scalars, points, normalisation, 28-bit copy; the host blocks in the
// pageable copies) while the main stream multiplies the piece before, out of workspaces instead of an SRS entry.  Measured at 2^20
// pairs: the three calls 8.9 ms (upload 2.7 + normalise 1.1 + allocations, multiply 4.6 with the scalars' upload, free 0.4); one piece
// 8.6, two pieces 8.3, three 10.2, four 11.6 -- a multiplication without tables pays ~0.8 ms of sort, running-sum reduction and
// host epilogue per piece whatever its size, so two pieces (BP_SEAM_PIECES: 1..4) are where the overlap still wins.
constexpr int SEAM_PIECES = 4;
static_assert(SEAM_PIECES <= MSM_SLOTS, "one pinned result slot per piece");
int bp_msm_g1_projective144(bp_ctx* ctx, const uint8_t* points144, size_t n_points, const void* scalars, size_t n_scalars, int scalar_fmt,
                            uint8_t out96[96]) {
  if (!ctx || !out96 || !fmt_ok(scalar_fmt) || (n_points && !points144) || (n_scalars && !scalars)) return BP_ERR_INVALID_ARG;
  const size_t n = std::min(n_points, n_scalars);
  if (is_group(ctx) || n < ((size_t)1 << 17)) {
    uint64_t h = 0;
    BP_TRY(bp_srs_load_projective144(ctx, points144, n, &h));
    int rc = bp_msm_g1(ctx, h, scalars, n, scalar_fmt, out96);
    const std::string msg = ctx->last_error;
    (void)bp_srs_free(ctx, h);
    if (rc != BP_OK) ctx->last_error = msg;
    return rc;
  }
  DeviceGuard guard(ctx->device);
  bp_ctx* side;
  BP_TRY(side_ctx_get(ctx, &side));
  hipEvent_t* seam_ev;                                     // [k]: piece k uploaded and normalised (recorded on the side stream)
  BP_TRY(ev_get(ctx, "seam", SEAM_PIECES, hipEventDisableTiming, &seam_ev));
  int pieces = 2;
  {
    const char* v = knob("BP_SEAM_PIECES");
    if (v && *v >= '1' && *v <= '0' + SEAM_PIECES && !v[1]) pieces = *v - '0';
  }
  const size_t piece = (n + pieces - 1) / pieces;
  uint8_t* d_proj;
  g1_affine* d_aff;
  g1_affine28* d_p28;
  fr_t* d_scal;
  BP_TRY(ws_get(ctx, "seam.proj", piece * 144, (void**)&d_proj));
  BP_TRY(ws_get(ctx, "seam.affine", n * sizeof(g1_affine), (void**)&d_aff));
  BP_TRY(ws_get(ctx, "seam.p28", n * sizeof(g1_affine28), (void**)&d_p28));
  BP_TRY(ws_get(ctx, "seam.scalars", n * sizeof(fr_t), (void**)&d_scal));
  BP_HIP(ctx, stream_wait(ctx->stream));                 // the workspaces may still be read by work the caller enqueued before
  MsmPending pend[SEAM_PIECES];
  int launched = 0, rc = BP_OK;
  for (int k = 0; k < pieces && rc == BP_OK; k++) {
    const size_t lo = (size_t)k * piece, cnt = lo < n ? std::min(piece, n - lo) : 0;
    if (!cnt) break;
    hipError_t he = hipMemcpyAsync(d_scal + lo, (const uint8_t*)scalars + lo * 32, cnt * 32, hipMemcpyHostToDevice, side->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(d_proj, points144 + lo * 144, cnt * 144, hipMemcpyHostToDevice, side->stream);
    if (he != hipSuccess) {
      rc = fail(ctx, BP_ERR_HIP, "bucket_msm operands upload", he, __FILE__, __LINE__);
      break;
    }
    rc = srs_from_projective_run(side, (const g1_proj*)d_proj, cnt, d_aff + lo);
    if (rc == BP_OK) rc = srs_to28_into(side, d_aff + lo, cnt, d_p28 + lo);
    if (rc != BP_OK) {
      ctx->last_error = side->last_error;
      break;
    }
    he = hipEventRecord(seam_ev[k], side->stream);
    if (he == hipSuccess) he = hipStreamWaitEvent(ctx->stream, seam_ev[k], 0);
    if (he != hipSuccess) {
      rc = fail(ctx, BP_ERR_HIP, "bucket_msm piece order", he, __FILE__, __LINE__);
      break;
    }
    rc = msm_launch(ctx, d_p28 + lo, cnt, d_scal + lo, scalar_fmt, 0, 0, k, nullptr, &pend[k]);
    if (rc == BP_OK) launched = k + 1;
  }
  // every launched piece is finished (waited for) even after an error: the pinned slots and workspaces must be quiet on return
  g1_proj acc = g1_identity();
  uint64_t adds = 0;
  for (int k = 0; k < launched; k++) {
    g1_proj part;
    const int r2 = msm_finish(ctx, pend[k], &part);
    if (r2 != BP_OK && rc == BP_OK) rc = r2;
    if (r2 == BP_OK) {
      g1_add(acc, acc, part);
      adds += pend[k].adds;
    }
  }
  if (rc != BP_OK) {
    (void)stream_wait(side->stream);
    return rc;
  }
  ctx->msm_adds = adds;
  host_encode96(out96, acc);
  return BP_OK;
}

// one MSM of a plain context against its SRS whose result stays in HBM as a record; wait: finish it (status, stats) before returning
static int msm_blob_device(bp_ctx* ctx, uint64_t srs_handle, size_t first, const void* scalars, size_t n_scalars, int scalar_fmt,
                           int scalars_on_device, void* d_blob, bool wait) {
  if (!ctx || !d_blob || !fmt_ok(scalar_fmt) || (n_scalars && !scalars)) return BP_ERR_INVALID_ARG;
  if (is_group(ctx)) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "blob records are the one-process-per-GPU exchange; a bp_init_multi context combines its shards itself");
  SrsEntry* e;
  BP_TRY(srs_find(ctx, srs_handle, &e));
  if (first > e->n) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "SRS offset out of bounds");
  const size_t n = std::min(n_scalars, e->n - first);
  DeviceGuard guard(ctx->device);
  MsmPending pend;
  BP_TRY(msm_shard_launch(ctx, e, first, scalars, n, scalar_fmt, scalars_on_device ? 1 : 0, ctx->device, nullptr, 0, d_blob, &pend));
  if (wait) return msm_finish(ctx, pend, nullptr);
  // nothing is waited for: the stats of this MSM are read from its events by bp_msm_last_stats once the stream has passed them
  ctx->msm_async_pending = !pend.empty;
  ctx->msm_c = pend.c;
  ctx->msm_tables = pend.tables;
  ctx->msm_adds = pend.adds;
  if (pend.empty) ctx->msm_accumulate_ms = ctx->msm_total_ms = 0;
  return BP_OK;
}
int bp_msm_g1_blob_device(bp_ctx* ctx, uint64_t srs_handle, size_t first, const void* scalars, size_t n_scalars, int scalar_fmt,
                          int scalars_on_device, void* d_blob) {
  return msm_blob_device(ctx, srs_handle, first, scalars, n_scalars, scalar_fmt, scalars_on_device, d_blob, true);
}
int bp_msm_g1_blob_device_async(bp_ctx* ctx, uint64_t srs_handle, size_t first, const void* scalars, size_t n_scalars, int scalar_fmt,
                                int scalars_on_device, void* d_blob) {
  return msm_blob_device(ctx, srs_handle, first, scalars, n_scalars, scalar_fmt, scalars_on_device, d_blob, false);
}

int bp_msm_blobs_sum_device(bp_ctx* ctx, const void* d_blobs, size_t n_blobs, void* d_out_blob) {
  if (!ctx || !d_blobs || !d_out_blob || n_blobs == 0 || n_blobs > 4096) return BP_ERR_INVALID_ARG;
  DeviceGuard guard(ctx->device);
  return msm_blobs_sum_device_run(ctx, d_blobs, n_blobs, d_out_blob);
}
int bp_msm_blobs_sum_device_async(bp_ctx* ctx, const void* d_blobs, size_t n_blobs, void* d_out_blob) {
  if (!ctx || !d_blobs || !d_out_blob || n_blobs == 0 || n_blobs > 4096) return BP_ERR_INVALID_ARG;
  DeviceGuard guard(ctx->device);
  return msm_blobs_sum_device_run(ctx, d_blobs, n_blobs, d_out_blob, false);
}

int bp_msm_blobs_combine(const void* blobs, size_t n_blobs, uint8_t out96[96]) {
  if (!out96 || (n_blobs && !blobs)) return BP_ERR_INVALID_ARG;
  g1_proj r;
  BP_TRY(msm_blobs_combine((const uint8_t*)blobs, n_blobs, &r));
  host_encode96(out96, r);
  return BP_OK;
}

int bp_msm_window_scalars(const void* scalars, size_t n, int scalar_fmt, size_t b, size_t c, void* out_le32) {
  if (!fmt_ok(scalar_fmt) || (n && (!scalars || !out_le32)) || c == 0 || c > 63) return BP_ERR_INVALID_ARG;
  const size_t k = b / c;
  if (k == 0 || k * c > 256) return BP_ERR_INVALID_ARG;
  const size_t shift = 256 - k * c, words = shift / 32, bits = shift % 32;
  const uint8_t* in = (const uint8_t*)scalars;
  uint8_t* out = (uint8_t*)out_le32;
  for (size_t i = 0; i < n; i++) {
    fr_t v, r;
    memcpy(&v, in + 32 * i, 32);
    if (scalar_fmt == BP_FR_MONT) {
      Fr::from_mont(v, v);                                // Scalar::to_bytes (scalar.rs:292-304)
    } else {
      fr_t t;
      if (!big_sub(t, v, Fr::modulus())) return BP_ERR_BAD_SCALAR;
    }
    for (size_t j = 0; j < 8; j++) {
      const uint64_t lo = j + words < 8 ? v.l[j + words] : 0u, hi = j + words + 1 < 8 ? v.l[j + words + 1] : 0u;
      r.l[j] = (uint32_t)(((hi << 32) | lo) >> bits);
    }
    memcpy(out + 32 * i, &r, 32);
  }
  return BP_OK;
}

int bp_g1_sum_partials(const uint8_t* partials144, size_t n, uint8_t out96[96]) {
  if (!out96 || (n && !partials144)) return BP_ERR_INVALID_ARG;
  g1_proj acc = g1_identity();
  for (size_t i = 0; i < n; i++) {
    g1_proj p;
    memcpy(&p, partials144 + 144 * i, 144);
    g1_add(acc, acc, p);
  }
  host_encode96(out96, acc);
  return BP_OK;
}
int bp_g1_partial_to_bytes96(const uint8_t in144[144], uint8_t out96[96]) { return bp_g1_sum_partials(in144, 1, out96); }
int bp_g1_bytes96_to_partial(const uint8_t in96[96], uint8_t out144[144]) {
  if (!in96 || !out144) return BP_ERR_INVALID_ARG;
  g1_proj p;
  if (!host_decode96(p, in96)) return BP_ERR_BAD_POINT;
  memcpy(out144, &p, 144);
  return BP_OK;
}

int bp_g1_bytes96_to_compressed48(const uint8_t in96[96], uint8_t out48[48]) {
  if (!in96 || !out48) return BP_ERR_INVALID_ARG;
  g1_proj p;
  if (!host_decode96(p, in96)) return BP_ERR_BAD_POINT;
  host_compress48(out48, p);
  return BP_OK;
}
int bp_msm_last_member_stats(bp_ctx* ctx, int member, float* upload_ms, float* accumulate_ms, float* total_device_ms, uint64_t* mixed_adds) {
  if (!ctx) return BP_ERR_INVALID_ARG;
  const std::vector<bp_ctx*> sh = shards_of(ctx);
  if (member < 0 || (size_t)member >= sh.size()) return BP_ERR_INVALID_ARG;
  const bp_ctx* m = sh[member];
  if (upload_ms) *upload_ms = m->msm_upload_ms;
  const bool group = sh.size() > 1;
  if (accumulate_ms) *accumulate_ms = group ? m->shard_accumulate_ms : m->msm_accumulate_ms;
  if (total_device_ms) *total_device_ms = group ? m->shard_total_ms : m->msm_total_ms;
  if (mixed_adds) *mixed_adds = group ? m->shard_adds : m->msm_adds;
  return BP_OK;
}
int bp_msm_last_path(bp_ctx* ctx, int member, uint32_t out[12]) {
  if (!ctx || !out) return BP_ERR_INVALID_ARG;
  const std::vector<bp_ctx*> sh = shards_of(ctx);
  if (member < 0 || (size_t)member >= sh.size()) return BP_ERR_INVALID_ARG;
  memcpy(out, sh[member]->msm_path, sizeof sh[member]->msm_path);
  return BP_OK;
}
int bp_msm_last_used_tables(bp_ctx* ctx) { return ctx ? (ctx->msm_tables ? 1 : 0) : BP_ERR_INVALID_ARG; }
int bp_msm_last_stats(bp_ctx* ctx, float* accumulate_ms, float* total_device_ms, uint64_t* mixed_adds, uint32_t* window_bits) {
  if (!ctx) return BP_ERR_INVALID_ARG;
  if (ctx->msm_async_pending) {        // the last MSM was only enqueued: its events are read now (0 while it is still running)
    DeviceGuard guard(ctx->device);
    float a = 0, t = 0;
    if (hipEventElapsedTime(&a, ctx->ev[1], ctx->ev[2]) == hipSuccess && hipEventElapsedTime(&t, ctx->ev[0], ctx->ev[3]) == hipSuccess) {
      ctx->msm_accumulate_ms = a;
      ctx->msm_total_ms = t;
      ctx->msm_async_pending = false;
    } else {
      (void)hipGetLastError();
      ctx->msm_accumulate_ms = ctx->msm_total_ms = 0;
    }
  }
  if (accumulate_ms) *accumulate_ms = ctx->msm_accumulate_ms;
  if (total_device_ms) *total_device_ms = ctx->msm_total_ms;
  if (mixed_adds) *mixed_adds = ctx->msm_adds;
  if (window_bits) *window_bits = ctx->msm_c;
  return BP_OK;
}

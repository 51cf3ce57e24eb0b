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

namespace bp {
// the launch-and-finish rule of ctx.hpp
int msm_finish_all(bp_ctx* ctx, MsmFlight* f, size_t count, int rc) {
  const std::string launch_error = rc != BP_OK ? ctx->last_error : std::string();
  auto launched = [&](size_t i) { return f[i].launched; };
  auto finish = [&](size_t i) {
    DeviceGuard guard(f[i].on->device);
    f[i].rc = msm_finish(f[i].on, f[i].pend, f[i].out);
  };
  // In a group the waits and the host epilogues (window sums -> Horner, ~0.1 ms each) run on the members' own threads: eight in
  // sequence would cost more than the shards' GPU time of a 2^20-point MSM split eight ways.
  bool by_member = is_group(ctx) && count == ctx->members.size();
  for (size_t r = 0; r < count && by_member; r++) by_member = f[r].on == ctx->members[r];
  if (by_member) {
    over_members(ctx, count, launched, finish);
  } else {
    for (size_t i = 0; i < count; i++)
      if (launched(i)) finish(i);
  }
  if (rc != BP_OK) {
    ctx->last_error = launch_error;
    return rc;
  }
  for (size_t i = 0; i < count; i++)
    if (launched(i) && f[i].rc != BP_OK) return lift(ctx, f[i].on, f[i].rc);
  return BP_OK;
}
}  // namespace bp

// Member m's slices of vectors that live in the HBM of the leader's device: once the leader's stream has reached `ready`, slice j
// (len[j] scalars from src[j]) is copied GPU to GPU into the member's workspace, the slices back to back; at[j] = where it lies there.
static int slices_from_leader(bp_ctx* m, int leader_device, hipEvent_t ready, int cnt, const fr_t* const* src, const size_t* len, const fr_t** at) {
  size_t total = 0;
  for (int j = 0; j < cnt; j++) total += len[j];
  fr_t* d;
  BP_TRY(ws_get(m, "io.scalars", total * sizeof(fr_t), (void**)&d));
  BP_HIP(m, hipStreamWaitEvent(m->stream, ready, 0));
  for (int j = 0; j < cnt; d += len[j++]) {
    at[j] = d;
    if (!len[j]) continue;
    if (!peer_path(m, leader_device)) BP_HIP(m, hipMemcpyAsync(d, src[j], len[j] * sizeof(fr_t), hipMemcpyDeviceToDevice, m->stream));
    else BP_HIP(m, hipMemcpyPeerAsync(d, m->device, src[j], leader_device, len[j] * sizeof(fr_t), m->stream));
  }
  return BP_OK;
}

// Enqueue the MSM of one shard: scalars[0..n) against the member's points [local_first, local_first + n).
//   where 0: `scalars` is host memory; 1: HBM of this member's device; 2: HBM of device src_device (the leader's), behind `ready`
static int msm_shard_launch(bp_ctx* m, SrsEntry* e, size_t local_first, const void* scalars, size_t n, int fmt, int where, int src_device,
                            hipEvent_t ready, int slot, void* d_blob, MsmPending* pend) {
  DeviceGuard guard(m->device);
  const fr_t *d_scalars = (const fr_t*)scalars, *src = d_scalars;
  if (where == 0 && n) {
    fr_t* d;
    BP_TRY(ws_get(m, "io.scalars", n * sizeof(fr_t), (void**)&d));
    BP_HIP(m, hipEventRecord(m->ev[4], m->stream));            // upload = ev[4] .. ev[0] (msm_launch records ev[0] first thing)
    BP_HIP(m, hipMemcpyAsync(d, scalars, n * sizeof(fr_t), hipMemcpyHostToDevice, m->stream));
    d_scalars = d;
  } else if (where == 2 && n) {
    BP_TRY(slices_from_leader(m, src_device, ready, 1, &src, &n, &d_scalars));
  }
  if (srs_tables_pay(*e, n)) return msm_launch(m, e->d_table + local_first, n, d_scalars, fmt, e->table_c, e->n, slot, d_blob, pend);
  return msm_launch(m, e->d_points28 + local_first, n, d_scalars, fmt, 0, 0, slot, d_blob, pend);
}

// sum_{i < n} s_i P_{first + i} over the shards sh of an SRS (srs_shards), in two steps so that several such sums can be in flight:
// launch enqueues every shard's whole pipeline (result slot `slot` of each member; f[r] is member r's), finish waits and adds the
// partial sums.  More scalars than points: cut to the SRS (shard_cut).
static int msm_all_shards_launch(bp_ctx* ctx, const std::vector<SrsShard>& sh, size_t first, const void* scalars, size_t n_scalars, int scalar_fmt,
                                 int scalars_on_device, int slot, MsmFlight* f) {
  const size_t R = sh.size();
  for (size_t r = 0; r < R; r++) f[r].on = sh[r].m;
  if (R > 1 && scalars_on_device) {            // the members' copies must see what the leader's stream has produced
    DeviceGuard guard(ctx->device);
    BP_HIP(ctx, hipEventRecord(ctx->ev[4], ctx->stream));
  }
  // a shard none of the range lies on is skipped -- except the only shard of a plain context: the empty MSM resets the stats and yields the identity
  auto cut = [&](size_t r, size_t* lo, size_t* hi) {
    shard_cut(first, n_scalars, sh[0].e->n_global, sh[r].e->first, sh[r].e->n, lo, hi);
    return *lo < *hi || R == 1;
  };
  auto take = [&](size_t r) {
    size_t lo, hi;
    return cut(r, &lo, &hi);
  };
  auto launch_one = [&](size_t r) {
    const SrsShard& s = sh[r];
    size_t lo, hi;
    cut(r, &lo, &hi);
    const bool any = lo < hi;
    const int where = !scalars_on_device ? 0 : (r == 0 ? 1 : 2);
    msm_flight_launched(f[r], s.m, msm_shard_launch(s.m, s.e, any ? lo - s.e->first : 0, (const uint8_t*)scalars + (any ? (lo - first) * sizeof(fr_t) : 0),
                                                    any ? hi - lo : 0, scalar_fmt, where, ctx->device, ctx->ev[4], slot, nullptr, &f[r].pend));
  };
  // the launches: scalars already in HBM are enqueued by this thread (asynchronous copies and kernels);
  // host scalars go through the members' own threads, so that the uploads -- staged by the issuing thread when the memory is
  // pageable, as a Rust Vec<Scalar> is -- run on all PCIe links at once instead of one after another
  if (!scalars_on_device && R > 1) {
    over_members(ctx, R, take, launch_one);
  } else {
    for (size_t r = 0; r < R; r++)
      if (take(r)) launch_one(r);
  }
  for (size_t r = 0; r < R; r++)
    if (f[r].rc != BP_OK) return lift(ctx, f[r].on, f[r].rc);
  return BP_OK;               // either way the caller finishes whatever was launched
}
static int msm_all_shards_finish(bp_ctx* ctx, MsmFlight* f, size_t R, bool host_scalars, int rc, g1_proj* out) {
  rc = msm_finish_all(ctx, f, R, rc);
  g1_proj acc = g1_identity();
  float acc_ms = 0, dev_ms = 0;
  uint64_t adds = 0;
  for (size_t r = 0; r < R; r++) {
    if (!f[r].launched) continue;
    bp_ctx* m = f[r].on;
    m->shard_accumulate_ms = m->msm_accumulate_ms;
    m->shard_total_ms = m->msm_total_ms;
    m->shard_adds = m->msm_adds;
    m->msm_upload_ms = 0;
    if (f[r].rc != BP_OK) continue;
    if (host_scalars && !f[r].pend.empty) {
      DeviceGuard guard(m->device);
      if (hipEventElapsedTime(&m->msm_upload_ms, m->ev[4], m->ev[0]) != hipSuccess) {
        (void)hipGetLastError();
        m->msm_upload_ms = 0;
      }
    }
    if (R == 1) acc = f[r].out[0]; else g1_add(acc, acc, f[r].out[0]);
    acc_ms = std::max(acc_ms, m->msm_accumulate_ms);
    dev_ms = std::max(dev_ms, m->msm_total_ms);
    adds += m->msm_adds;
  }
  if (rc != BP_OK) return rc;
  if (R > 1) {                                   // stats of a group: the slowest shard, all additions
    ctx->msm_accumulate_ms = acc_ms;
    ctx->msm_total_ms = dev_ms;
    ctx->msm_adds = adds;
  }
  *out = acc;
  return BP_OK;
}
static int msm_all_shards(bp_ctx* ctx, uint64_t srs_handle, size_t first, const void* scalars, size_t n_scalars, int scalar_fmt,
                          int scalars_on_device, g1_proj* out) {
  std::vector<SrsShard> sh;
  BP_TRY(srs_shards(ctx, srs_handle, &sh));
  if (first > sh[0].e->n_global) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "SRS offset out of bounds");
  std::vector<MsmFlight> f(sh.size());
  const int rc = msm_all_shards_launch(ctx, sh, first, scalars, n_scalars, scalar_fmt, scalars_on_device, 0, f.data());
  return msm_all_shards_finish(ctx, f.data(), f.size(), !scalars_on_device, rc, out);
}


namespace bp {
// One round of COMMIT_GROUP_BATCH: cnt commitments of HBM-resident coefficient vectors (on the leader) over the members of a group.
// Every member that holds a part of them receives its slice of each (slices_from_leader), runs ONE pipeline over the slices' bucket
// sets and delivers one partial sum per vector; the host adds the members' partial sums.
static int commit_group_batch_round(bp_ctx* ctx, const std::vector<SrsShard>& sh, const CommitShard* cs, const fr_t* const* d_coeffs, const size_t* n,
                                    int cnt, g1_proj* out) {
  const size_t R = sh.size();
  {
    DeviceGuard guard(ctx->device);
    BP_HIP(ctx, hipEventRecord(ctx->ev[4], ctx->stream));          // the coefficient vectors were produced on the leader's stream
  }
  std::vector<MsmFlight> f(R);
  for (size_t r = 0; r < R; r++) f[r].on = sh[r].m;
  int rc = BP_OK;
  for (size_t r = 0; r < R && rc == BP_OK; r++) {
    bp_ctx* m = sh[r].m;
    const SrsEntry* e = sh[r].e;
    DeviceGuard guard(m->device);
    const fr_t *src[MSM_MAX_BATCH], *ptrs[MSM_MAX_BATCH];
    size_t lens[MSM_MAX_BATCH];
    if (commit_slices(cs[r], sh[0].e->n_global, n, cnt, lens) == 0) continue;
    for (int j = 0; j < cnt; j++) ptrs[j] = src[j] = d_coeffs[j] + (lens[j] ? e->first : 0);
    int rc1 = r == 0 ? BP_OK : slices_from_leader(m, ctx->device, ctx->ev[4], cnt, src, lens, ptrs);
    if (rc1 == BP_OK) rc1 = msm_launch_many(m, e->d_table, (uint32_t)cnt, ptrs, lens, BP_FR_MONT, e->table_c, e->n, 0, nullptr, &f[r].pend);
    rc = lift(ctx, m, msm_flight_launched(f[r], m, rc1));
  }
  BP_TRY(msm_finish_all(ctx, f.data(), R, rc));
  for (int j = 0; j < cnt; j++) {
    g1_proj acc = g1_identity();
    for (size_t r = 0; r < R; r++)
      if (f[r].launched) g1_add(acc, acc, f[r].out[j]);
    out[j] = acc;
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
// one commitment on a lane, behind `ready` (nullptr: the lane's own stream order is enough)
static int lane_launch(bp_ctx* ctx, bp_ctx* lane, SrsEntry* e, const fr_t* d_coeffs, size_t n, hipEvent_t ready, MsmFlight* f) {
  f->on = lane;
  if (ready) BP_HIP(ctx, hipStreamWaitEvent(lane->stream, ready, 0));
  const int rc = msm_shard_launch(lane, e, 0, d_coeffs, shard_slice(n, e->n_global, e->first, e->n), BP_FR_MONT, 1, ctx->device, nullptr, 0, nullptr, &f->pend);
  return lift(ctx, lane, msm_flight_launched(*f, lane, rc));
}

static int commit_batch_knob() {
  const char* v = knob("BP_COMMIT_BATCH");
  return !v ? COMMIT_KNOB_UNSET : *v == '0' ? 0 : *v == '1' ? 1 : COMMIT_KNOB_UNSET;
}

// Setup::commit, k times: the route and its rounds are commit_plan's (commit_plan.hpp); each case below runs the rounds of one route.
int commit_many(bp_ctx* ctx, uint64_t srs_handle, const fr_t* const* d_coeffs, const size_t* n, int k, g1_proj* out) {
  if (k <= 0) return BP_OK;
  std::vector<SrsShard> sh;
  BP_TRY(srs_shards(ctx, srs_handle, &sh));
  const size_t R = sh.size();
  SrsEntry* e = sh[0].e;
  std::vector<CommitShard> cs(R);
  for (size_t r = 0; r < R; r++) cs[r] = {sh[r].e->first, sh[r].e->n, sh[r].e->d_table ? sh[r].e->table_c : 0u};
  const CommitPlan plan = commit_plan(cs.data(), R, e->n_global, k, n, is_group(ctx), commit_batch_knob(), msm_knobs());
  switch (plan.route) {
    case COMMIT_GROUP_BATCH:
      for (const CommitRound& rd : plan.rounds) BP_TRY(commit_group_batch_round(ctx, sh, cs.data(), d_coeffs + rd.base, n + rd.base, rd.cnt, out + rd.base));
      return BP_OK;
    case COMMIT_SHARDED:
      for (const CommitRound& rd : plan.rounds) {            // every member queues its shards of the round's commitments back to back
        std::vector<MsmFlight> f(R * rd.cnt);
        int rcs[MSM_SLOTS], tried = 0, rc = BP_OK;
        for (; tried < rd.cnt && rc == BP_OK; tried++)
          rcs[tried] = rc = msm_all_shards_launch(ctx, sh, 0, d_coeffs[rd.base + tried], n[rd.base + tried], BP_FR_MONT, 1, tried, &f[R * tried]);
        for (int j = 0; j < tried; j++) {
          const int rc1 = msm_all_shards_finish(ctx, &f[R * j], R, false, rcs[j], &out[rd.base + j]);
          if (rc == BP_OK) rc = rc1;
        }
        BP_TRY(rc);
      }
      return BP_OK;
    case COMMIT_DEVICE_BATCH: {
      DeviceGuard guard(ctx->device);
      for (const CommitRound& rd : plan.rounds) {
        size_t lens[MSM_MAX_BATCH];
        commit_slices(cs[0], e->n_global, n + rd.base, rd.cnt, lens);
        MsmPending pend;
        BP_TRY(msm_launch_many(ctx, e->d_table, (uint32_t)rd.cnt, d_coeffs + rd.base, lens, BP_FR_MONT, e->table_c, e->n, 0, nullptr, &pend));
        BP_TRY(msm_finish(ctx, pend, &out[rd.base]));
      }
      return BP_OK;
    }
    case COMMIT_LANES: {
      DeviceGuard guard(ctx->device);
      bp_ctx* last;
      BP_TRY(lane_get(ctx, plan.width < k ? plan.width - 1 : k - 1, &last));      // every lane the rounds below use exists before the first launch
      for (const CommitRound& rd : plan.rounds) {
        BP_HIP(ctx, hipEventRecord(ctx->ev[4], ctx->stream));          // the coefficient vectors were produced on ctx->stream
        MsmFlight f[MAX_LANES];
        int rc = BP_OK;
        for (int j = 0; j < rd.cnt && rc == BP_OK; j++)
          rc = lane_launch(ctx, lane_of(ctx, j), e, d_coeffs[rd.base + j], n[rd.base + j], j ? ctx->ev[4] : nullptr, &f[j]);
        rc = msm_finish_all(ctx, f, rd.cnt, rc);
        for (int j = 0; j < rd.cnt; j++) {
          if (!f[j].launched || f[j].rc != BP_OK) continue;
          out[rd.base + j] = f[j].out[0];
          if (f[j].on->msm_accumulate_ms > ctx->msm_accumulate_ms) ctx->msm_accumulate_ms = f[j].on->msm_accumulate_ms;
        }
        BP_TRY(rc);
      }
      return BP_OK;
    }
  }
  return BP_ERR_INVALID_ARG;
}

int commit_lane_launch(bp_ctx* ctx, int j, uint64_t srs_handle, const fr_t* d_coeffs, size_t n, hipEvent_t ready, MsmPending* pend) {
  *pend = MsmPending();
  if (j < 0 || j >= MAX_LANES || is_group(ctx)) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "commit lane");
  SrsEntry* e;
  BP_TRY(srs_find(ctx, srs_handle, &e));
  DeviceGuard guard(ctx->device);
  bp_ctx* lane;
  BP_TRY(lane_get(ctx, j, &lane));
  MsmFlight f;
  const int rc = lane_launch(ctx, lane, e, d_coeffs, n, ready, &f);
  *pend = f.pend;
  return rc;
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
  MsmFlight f[SEAM_PIECES];
  int rc = BP_OK;
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
    rc = msm_flight_launched(f[k], ctx, msm_launch(ctx, d_p28 + lo, cnt, d_scal + lo, scalar_fmt, 0, 0, k, nullptr, &f[k].pend));
  }
  rc = msm_finish_all(ctx, f, pieces, rc);
  if (rc != BP_OK) {
    (void)stream_wait(side->stream);
    return rc;
  }
  g1_proj acc = g1_identity();
  uint64_t adds = 0;
  for (int k = 0; k < pieces; k++) {
    if (!f[k].launched) continue;
    g1_add(acc, acc, f[k].out[0]);
    adds += f[k].pend.adds;
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

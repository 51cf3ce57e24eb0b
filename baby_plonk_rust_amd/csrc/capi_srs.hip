// capi_srs.hip -- C ABI, part 2a: the SRS store (Setup.powers_of_x resident in HBM): load in three encodings, generate, export,
// subgroup check, free, and the fixed-base tables with their memory budget.  One context holds one shard per member of a group;
// srs_shards below is the one place that maps a handle to its shards and a point range to each shard's part of it.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "ctx.hpp"
#include "g1_check.hpp"
#include "g1_ntt.hpp"

#include "capi_common.hpp"

using namespace bp;

// takes ownership of d (freed on failure); the entry covers global points [first, first + n) of an SRS of n_global points
int srs_register(bp_ctx* ctx, g1_affine* d, size_t n, size_t first, size_t n_global, uint64_t* handle) {
  SrsEntry e;
  e.d_points = d;
  e.n = n;
  e.first = first;
  e.n_global = n_global;
  int rc = srs_to28_run(ctx, d, n, &e.d_points28);
  if (rc == BP_OK && stream_wait(ctx->stream) != hipSuccess) rc = fail(ctx, BP_ERR_HIP, "srs_to28", hipGetLastError(), __FILE__, __LINE__);
  if (rc != BP_OK) {
    (void)hipFree(d);
    if (e.d_points28) (void)hipFree(e.d_points28);
    return rc;
  }
  *handle = ctx->next_handle++;
  ctx->srs[*handle] = e;
  return BP_OK;
}
int srs_find(bp_ctx* ctx, uint64_t handle, SrsEntry** out) {
  auto it = ctx->srs.find(handle);
  if (it == ctx->srs.end()) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "unknown SRS handle");
  *out = &it->second;
  return BP_OK;
}
// The one walk from a handle to its shards (capi_common.hpp): member r's entry under the handle the leader's entry lists for it
// (a plain context has only its own), and the part of [first, first + n) on it (shard_cut, commit_plan.hpp).
int srs_shards(bp_ctx* ctx, uint64_t srs_handle, std::vector<SrsShard>* out, size_t first, size_t n) {
  SrsEntry* lead;
  BP_TRY(srs_find(ctx, srs_handle, &lead));
  const std::vector<bp_ctx*> sh = shards_of(ctx);
  out->resize(sh.size());
  for (size_t r = 0; r < sh.size(); r++) {
    SrsShard& s = (*out)[r];
    s.m = sh[r];
    s.handle = lead->member_handle.empty() ? srs_handle : lead->member_handle[r];
    BP_TRY(lift(ctx, s.m, srs_find(s.m, s.handle, &s.e)));
    shard_cut(first, n, lead->n_global, s.e->first, s.e->n, &s.lo, &s.hi);
  }
  return BP_OK;
}
int srs_shards_checked(bp_ctx* ctx, uint64_t srs_handle, size_t first, size_t n, std::vector<SrsShard>* out) {
  BP_TRY(srs_shards(ctx, srs_handle, out, first, n));
  const size_t n_global = (*out)[0].e->n_global;
  if (first > n_global || n > n_global - first) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "SRS range out of bounds");
  return BP_OK;
}

int srs_free_one(bp_ctx* ctx, uint64_t handle) {
  SrsEntry* e;
  BP_TRY(srs_find(ctx, handle, &e));
  DeviceGuard guard(ctx->device);
  BP_HIP(ctx, stream_wait(ctx->stream));
  BP_HIP(ctx, hipFree(e->d_points));
  BP_HIP(ctx, hipFree(e->d_points28));
  if (e->d_table) BP_HIP(ctx, hipFree(e->d_table));
  if (e->d_open_all) BP_HIP(ctx, hipFree(e->d_open_all));
  ctx->srs.erase(handle);
  return BP_OK;
}

// bytes per host record of the SRS kinds that upload one (0, 1, 4)
static size_t srs_record_bytes(int kind) { return kind == 0 ? 96 : kind == 1 ? 144 : 48; }
// BP_ERR_BAD_POINT naming global point `index` and the reason of the status word (g1_check.hpp)
static int srs_bad_point(bp_ctx* ctx, uint64_t index, uint32_t reason, size_t* first_bad) {
  if (first_bad) *first_bad = (size_t)index;
  char msg[160];
  snprintf(msg, sizeof msg, "point %llu rejected: %s", (unsigned long long)index, g1_reject_text(reason, true));
  return BP_FAIL(ctx, BP_ERR_BAD_POINT, msg);
}

// One shard of an SRS on one device.  kind 0: decode 96-byte encodings, 1: normalise 144-byte projective images,
// 2: generate tau^i G, 3: generate (a + i d) G, 4: decode 48-byte compressed encodings (+ the subgroup test when checks has
// BP_SRS_CHECK_SUBGROUP; a rejected point's global index goes to *first_bad).  src: this shard's slice of the host input (kinds 0, 1, 4).
static int srs_make_one(bp_ctx* ctx, int kind, const uint8_t* src, const fr_t& a, const fr_t& d, size_t first, size_t n, size_t n_global,
                        uint64_t* handle, uint32_t checks = 0, size_t* first_bad = nullptr) {
  DeviceGuard guard(ctx->device);
  g1_affine* d_pts = nullptr;
  BP_HIP(ctx, hipMalloc((void**)&d_pts, std::max<size_t>(n, 1) * sizeof(g1_affine)));
  int rc = BP_OK;
  if (kind == 0 || kind == 1 || kind == 4) {
    const size_t rec = srs_record_bytes(kind);
    uint8_t* d_bytes = nullptr;
    rc = ws_get(ctx, "io.bytes", n * rec, (void**)&d_bytes);
    if (rc == BP_OK && n) {
      hipError_t e = hipMemcpyAsync(d_bytes, src, n * rec, hipMemcpyHostToDevice, ctx->stream);
      if (e != hipSuccess) rc = fail(ctx, BP_ERR_HIP, "SRS upload", e, __FILE__, __LINE__);
    }
    if (rc == BP_OK && kind == 4) {
      uint64_t bad = ~0ull;
      rc = srs_decode48_run(ctx, d_bytes, n, (checks & BP_SRS_CHECK_SUBGROUP) != 0, d_pts, &bad);
      if (rc == BP_OK && bad != ~0ull) rc = srs_bad_point(ctx, first + (bad >> 2), (uint32_t)(bad & 3), first_bad);
    } else if (rc == BP_OK) {
      rc = kind == 0 ? srs_decode_run(ctx, d_bytes, n, d_pts) : srs_from_projective_run(ctx, (const g1_proj*)d_bytes, n, d_pts);
    }
  } else {
    rc = srs_generate_run(ctx, a, d, kind == 2 ? 0 : 1, first, n, d_pts);
  }
  if (rc == BP_OK) {
    hipError_t e = stream_wait(ctx->stream);
    if (e != hipSuccess) rc = fail(ctx, BP_ERR_HIP, "SRS build", e, __FILE__, __LINE__);
  }
  if (rc != BP_OK) {
    (void)hipFree(d_pts);
    return rc;
  }
  return srs_register(ctx, d_pts, n, first, n_global, handle);
}

// the whole SRS: one shard per member (contiguous point ranges), the leader's entry lists the members' handles.
// Shards are built in ascending order and the first failing one ends the build, so *first_bad (kind 4) is the lowest global index.
static int srs_make(bp_ctx* ctx, int kind, const uint8_t* src, const fr_t& a, const fr_t& d, size_t n, uint64_t* handle, uint32_t checks = 0,
                    size_t* first_bad = nullptr) {
  const std::vector<bp_ctx*> sh = shards_of(ctx);
  const size_t rec = srs_record_bytes(kind);
  std::vector<uint64_t> hs;
  for (size_t r = 0; r < sh.size(); r++) {
    size_t lo, hi;
    shard_range(n, r, sh.size(), &lo, &hi);
    uint64_t h = 0;
    int rc = lift(ctx, sh[r], srs_make_one(sh[r], kind, src ? src + lo * rec : nullptr, a, d, lo, hi - lo, n, &h, checks, first_bad));
    if (rc != BP_OK) {
      for (size_t k = 0; k < hs.size(); k++) (void)srs_free_one(sh[k], hs[k]);
      return rc;
    }
    hs.push_back(h);
  }
  if (sh.size() > 1) ctx->srs[hs[0]].member_handle = hs;
  *handle = hs[0];
  return BP_OK;
}

int bp_srs_load(bp_ctx* ctx, const uint8_t* points96, size_t n, uint64_t* srs_handle) {
  if (!ctx || !srs_handle || (n && !points96)) return BP_ERR_INVALID_ARG;
  return srs_make(ctx, 0, points96, Fr::zero(), Fr::zero(), n, srs_handle);
}
int bp_srs_load_projective144(bp_ctx* ctx, const uint8_t* points144, size_t n, uint64_t* srs_handle) {
  if (!ctx || !srs_handle || (n && !points144)) return BP_ERR_INVALID_ARG;
  return srs_make(ctx, 1, points144, Fr::zero(), Fr::zero(), n, srs_handle);
}
int bp_srs_load_compressed48(bp_ctx* ctx, const uint8_t* points48, size_t n, uint32_t checks, uint64_t* srs_handle, size_t* first_bad) {
  if (first_bad) *first_bad = SIZE_MAX;
  if (!ctx || !srs_handle || (n && !points48) || (checks & ~BP_SRS_CHECK_SUBGROUP)) return BP_ERR_INVALID_ARG;
  return srs_make(ctx, 4, points48, Fr::zero(), Fr::zero(), n, srs_handle, checks, first_bad);
}

static int srs_generate_common(bp_ctx* ctx, size_t n, const uint8_t a32[32], const uint8_t d32[32], int mode, uint64_t* handle) {
  if (!ctx || !handle || !a32 || (mode == 1 && !d32)) return BP_ERR_INVALID_ARG;
  fr_t a, d = Fr::zero();
  if (!fr_from_bytes(a, a32, BP_FR_BYTES_LE)) return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, "scalar >= q");
  if (mode == 1 && !fr_from_bytes(d, d32, BP_FR_BYTES_LE)) return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, "scalar >= q");
  return srs_make(ctx, mode == 0 ? 2 : 3, nullptr, a, d, n, handle);
}
int bp_srs_generate(bp_ctx* ctx, size_t powers, const uint8_t tau32[32], uint64_t* srs_handle) {
  return srs_generate_common(ctx, powers, tau32, nullptr, 0, srs_handle);
}
int bp_srs_generate_progression(bp_ctx* ctx, size_t n, const uint8_t a32[32], const uint8_t d32[32], uint64_t* srs_handle) {
  return srs_generate_common(ctx, n, a32, d32, 1, srs_handle);
}

// The Lagrange-basis SRS over the 2^log_n-th roots of unity: L = i_ntt_381 over G1 of the first 2^log_n points (g1_ntt.hpp).  The
// transform runs on the context's own device (the leader's, for a group: the source's shards are collected there first, GPU to GPU as
// every group path moves data) and the result is dealt out in srs_make's point ranges, each shard registered like any other SRS.
int bp_srs_lagrange(bp_ctx* ctx, uint64_t srs_handle, uint32_t log_n, uint64_t* lagrange_handle) {
  if (!ctx || !lagrange_handle) return BP_ERR_INVALID_ARG;
  SrsEntry* lead;
  BP_TRY(srs_find(ctx, srs_handle, &lead));
  if (log_n > G1_NTT_MAX_LOG) return BP_FAIL(ctx, BP_ERR_TOO_LARGE, "log_n > 24");
  if (lead->basis != BP_BASIS_MONOMIAL) return BP_FAIL(ctx, BP_ERR_BASIS, "the source is itself a Lagrange SRS");
  const size_t n = (size_t)1 << log_n;
  if (n > lead->n_global) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "2^log_n exceeds the SRS's length");
  std::vector<SrsShard> sh;
  BP_TRY(srs_shards(ctx, srs_handle, &sh, 0, n));
  DeviceGuard guard(ctx->device);
  const g1_affine* d_src = sh[0].e->d_points;            // a plain context: the resident points as they are
  if (sh.size() > 1) {
    g1_affine* d_in;
    BP_TRY(ws_get(ctx, "srs.g1_ntt_in", n * sizeof(g1_affine), (void**)&d_in));
    for (const SrsShard& s : sh) {
      if (s.lo >= s.hi) continue;
      const g1_affine* part = s.e->d_points + (s.lo - s.e->first);
      const size_t bytes = (s.hi - s.lo) * sizeof(g1_affine);
      if (!peer_path(s.m, ctx->device)) BP_HIP(ctx, hipMemcpyAsync(d_in + s.lo, part, bytes, hipMemcpyDeviceToDevice, ctx->stream));
      else BP_HIP(ctx, hipMemcpyPeerAsync(d_in + s.lo, ctx->device, part, s.m->device, bytes, ctx->stream));
    }
    d_src = d_in;
  }
  g1_affine* d_full = nullptr;
  BP_HIP(ctx, hipMalloc((void**)&d_full, n * sizeof(g1_affine)));
  int rc = g1_ntt_run(ctx, d_src, log_n, d_full);         // waits for the stream: d_full is complete behind it
  if (rc != BP_OK) {
    (void)hipFree(d_full);
    return rc;
  }
  std::vector<uint64_t> hs;
  for (size_t r = 0; r < sh.size() && rc == BP_OK; r++) {
    bp_ctx* m = sh[r].m;
    size_t lo, hi;
    shard_range(n, r, sh.size(), &lo, &hi);
    uint64_t h = 0;
    if (sh.size() == 1) {
      rc = srs_register(ctx, d_full, n, 0, n, &h);        // takes d_full over
      d_full = nullptr;
    } else {
      DeviceGuard member(m->device);
      g1_affine* d_pts = nullptr;
      hipError_t he = hipMalloc((void**)&d_pts, std::max<size_t>(hi - lo, 1) * sizeof(g1_affine));
      if (he == hipSuccess && hi > lo)
        he = !peer_path(m, ctx->device) ? hipMemcpyAsync(d_pts, d_full + lo, (hi - lo) * sizeof(g1_affine), hipMemcpyDeviceToDevice, m->stream)
                                         : hipMemcpyPeerAsync(d_pts, m->device, d_full + lo, ctx->device, (hi - lo) * sizeof(g1_affine), m->stream);
      if (he != hipSuccess) {
        if (d_pts) (void)hipFree(d_pts);
        rc = fail(ctx, BP_ERR_HIP, "Lagrange SRS: shard to its member", he, __FILE__, __LINE__);
      } else {
        rc = lift(ctx, m, srs_register(m, d_pts, hi - lo, lo, n, &h));      // waits for m's stream: the copy is done behind it
      }
    }
    if (rc == BP_OK) {
      SrsEntry& e = m->srs[h];
      e.basis = BP_BASIS_LAGRANGE;
      e.log_n = log_n;
      hs.push_back(h);
    }
  }
  if (d_full) (void)hipFree(d_full);
  if (rc != BP_OK) {
    for (size_t k = 0; k < hs.size(); k++) (void)srs_free_one(sh[k].m, hs[k]);
    return rc;
  }
  if (sh.size() > 1) ctx->srs[hs[0]].member_handle = hs;
  *lagrange_handle = hs[0];
  return BP_OK;
}
int bp_srs_basis(bp_ctx* ctx, uint64_t srs_handle, int* basis, uint32_t* log_n) {
  if (!ctx) return BP_ERR_INVALID_ARG;
  SrsEntry* e;
  BP_TRY(srs_find(ctx, srs_handle, &e));
  if (basis) *basis = e->basis;
  if (log_n) *log_n = e->log_n;
  return BP_OK;
}
// INTERNAL, not part of include/bp_msm_ntt.h (tools/srs_lagrange_timing.py): the HIP-event time of each pass of the last
// bp_srs_lagrange on this context.  Writes min(cap, passes) values; *passes = the number of passes it ran.
extern "C" int bpx_srs_lagrange_pass_ms(bp_ctx* ctx, float* ms, uint32_t cap, uint32_t* passes) {
  if (!ctx || !passes || (cap && !ms)) return BP_ERR_INVALID_ARG;
  *passes = (uint32_t)ctx->g1_ntt_pass_ms.size();
  for (uint32_t i = 0; i < cap && i < *passes; i++) ms[i] = ctx->g1_ntt_pass_ms[i];
  return BP_OK;
}

int bp_srs_len(bp_ctx* ctx, uint64_t srs_handle, size_t* n) {
  if (!ctx || !n) return BP_ERR_INVALID_ARG;
  SrsEntry* e;
  BP_TRY(srs_find(ctx, srs_handle, &e));
  *n = e->n_global;
  return BP_OK;
}

// points [first, first + n) of every shard they lie on, encoded on the device: rec = 96 (to_uncompressed) or 48 (to_compressed)
static int srs_export_bytes(bp_ctx* ctx, uint64_t srs_handle, size_t first, size_t n, uint8_t* out, size_t rec) {
  std::vector<SrsShard> sh;
  BP_TRY(srs_shards_checked(ctx, srs_handle, first, n, &sh));
  for (const SrsShard& s : sh) {
    if (s.lo >= s.hi) continue;
    bp_ctx* m = s.m;
    const size_t cnt = s.hi - s.lo;
    DeviceGuard guard(m->device);
    uint8_t* d_bytes;
    BP_TRY(lift(ctx, m, ws_get(m, "io.bytes", cnt * rec, (void**)&d_bytes)));
    const g1_affine* src = s.e->d_points + (s.lo - s.e->first);
    BP_TRY(lift(ctx, m, rec == 96 ? srs_encode_run(m, src, cnt, d_bytes) : srs_encode48_run(m, src, cnt, d_bytes)));
    BP_HIP(ctx, hipMemcpyAsync(out + (s.lo - first) * rec, d_bytes, cnt * rec, hipMemcpyDeviceToHost, m->stream));
    BP_HIP(ctx, stream_wait(m->stream));
  }
  return BP_OK;
}
int bp_srs_export(bp_ctx* ctx, uint64_t srs_handle, size_t first, size_t n, uint8_t* points96) {
  if (!ctx || (n && !points96)) return BP_ERR_INVALID_ARG;
  return srs_export_bytes(ctx, srs_handle, first, n, points96, 96);
}
int bp_srs_export_compressed48(bp_ctx* ctx, uint64_t srs_handle, size_t first, size_t n, uint8_t* points48) {
  if (!ctx || (n && !points48)) return BP_ERR_INVALID_ARG;
  return srs_export_bytes(ctx, srs_handle, first, n, points48, 48);
}

int bp_srs_check_subgroup(bp_ctx* ctx, uint64_t srs_handle, size_t first, size_t n, size_t* first_bad) {
  if (first_bad) *first_bad = SIZE_MAX;
  if (!ctx) return BP_ERR_INVALID_ARG;
  std::vector<SrsShard> sh;
  BP_TRY(srs_shards_checked(ctx, srs_handle, first, n, &sh));
  for (const SrsShard& s : sh) {                      // shards in ascending point order: the first failing one holds the lowest index
    if (s.lo >= s.hi) continue;
    DeviceGuard guard(s.m->device);
    uint64_t bad = ~0ull;
    BP_TRY(lift(ctx, s.m, srs_subgroup_run(s.m, s.e->d_points + (s.lo - s.e->first), s.hi - s.lo, &bad)));
    if (bad != ~0ull) return srs_bad_point(ctx, s.lo + (bad >> 2), (uint32_t)(bad & 3), first_bad);
  }
  return BP_OK;
}

int bp_srs_export_projective144(bp_ctx* ctx, uint64_t srs_handle, size_t first, size_t n, uint8_t* points144) {
  if (!ctx || (n && !points144)) return BP_ERR_INVALID_ARG;
  std::vector<SrsShard> sh;
  BP_TRY(srs_shards_checked(ctx, srs_handle, first, n, &sh));
  for (const SrsShard& s : sh) {
    if (s.lo >= s.hi) continue;
    DeviceGuard guard(s.m->device);
    std::vector<g1_affine> aff(s.hi - s.lo);
    BP_HIP(ctx, hipMemcpyAsync(aff.data(), s.e->d_points + (s.lo - s.e->first), aff.size() * sizeof(g1_affine), hipMemcpyDeviceToHost, s.m->stream));
    BP_HIP(ctx, stream_wait(s.m->stream));
    for (size_t i = 0; i < aff.size(); i++) {                // G1Projective::from(&G1Affine) (g1.rs:176-190): z = 1, or the identity
      g1_proj p = g1_identity();
      if (!g1_affine_is_identity(aff[i])) {
        p.x = aff[i].x;
        p.y = aff[i].y;
        p.z = Fp::one();
      }
      memcpy(points144 + (s.lo - first + i) * 144, &p, 144);
    }
  }
  return BP_OK;
}

int bp_srs_free(bp_ctx* ctx, uint64_t srs_handle) {
  if (!ctx) return BP_ERR_INVALID_ARG;
  std::vector<SrsShard> sh;
  BP_TRY(srs_shards(ctx, srs_handle, &sh));
  int rc = BP_OK;
  for (size_t r = sh.size(); r-- > 0;) {                 // the leader's entry (r = 0) goes last: it names the others
    const int rc1 = lift(ctx, sh[r].m, srs_free_one(sh[r].m, sh[r].handle));
    if (rc == BP_OK) rc = rc1;
  }
  return rc;
}

static int srs_precompute_one(bp_ctx* ctx, SrsEntry* e, uint32_t c) {
  DeviceGuard guard(ctx->device);
  BP_HIP(ctx, stream_wait(ctx->stream));
  if (e->d_table) {
    BP_HIP(ctx, hipFree(e->d_table));
    e->d_table = nullptr;
    e->table_c = e->table_W = 0;
  }
  if (c == BP_SRS_TABLES_OFF) return BP_OK;
  BP_TRY(srs_tables_run(ctx, e->d_points, e->d_points28, e->n, c, &e->d_table, &e->table_W));
  e->table_c = c;
  return BP_OK;
}

bool srs_tables_pay(const SrsEntry& e, size_t n) { return e.d_table && srs_width_pays(e.table_c, n); }

int bp_srs_precompute(bp_ctx* ctx, uint64_t srs_handle, uint32_t window_bits) {
  if (!ctx) return BP_ERR_INVALID_ARG;
  std::vector<SrsShard> sh;
  BP_TRY(srs_shards(ctx, srs_handle, &sh));
  const SrsEntry* lead = sh[0].e;
  uint32_t c = window_bits;
  if (c == 0) c = srs_auto_width(lead->n);      // from the length of one shard (every shard of a group gets the same width)
  if (c != BP_SRS_TABLES_OFF && (c < 4 || c > 24))
    return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "window_bits must be 0 (auto), 1 (off) or 4..24");
  // Memory budget: the tables (rows x points x 128 B: 25.8 GB per GPU at 2^24 points) must fit beside whatever else lives on the
  // device -- a second prover context, the caller's tensors -- together with the workspaces the first MSM against them allocates.
  // The check comes BEFORE anything is released or allocated, and counts the bytes of the tables this SRS holds now as free (they
  // go once the new width is accepted): a refused explicit width therefore leaves the SRS exactly as it was, old tables included.
  // An automatic width that does not fit falls back to wider windows (fewer rows: 22 -> 12, 24 -> 11) -- but only to a width MSMs over
  // this SRS would use (srs_width_pays, the rule of msm_shard_launch: a 2^18-point SRS never builds 24-bit tables no MSM would touch) --
  // and then to NO tables (the MSM runs on the raw points, same bytes out: bp_srs_table_info reports what was built); an explicit
  // width that does not fit is an error that says how much is missing, not an out-of-memory failure halfway through the build.
  if (c == BP_SRS_TABLES_OFF) {
    for (const SrsShard& s : sh) BP_TRY(lift(ctx, s.m, srs_precompute_one(s.m, s.e, BP_SRS_TABLES_OFF)));
    return BP_OK;
  }
  auto fits = [&](uint32_t cc, size_t* need_out, size_t* free_out) -> int {
    std::map<int, size_t> per_device, held;              // shards that share a device (a rehearsal group) share its free memory
    for (const SrsShard& s : sh) {
      const SrsEntry* e = s.e;
      DeviceGuard guard(s.m->device);
      size_t free_b = 0, total_b = 0;
      BP_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
      if (ctx->free_bytes_probe) free_b = (size_t)ctx->free_bytes_probe;        // tests: the reading to decide on (bpx_set_free_bytes_probe below)
      const size_t rows = msm_windows(cc);
      size_t& need = per_device[s.m->device];
      size_t& old_bytes = held[s.m->device];
      if (e->d_table) old_bytes += (size_t)e->table_W * std::max<size_t>(e->n, 1) * sizeof(g1_affine28);
      need += rows * e->n * (sizeof(g1_affine28) + 24) + ((size_t)256 << 20);      // + sort records, lists, partial slots of one MSM
      if (need > free_b + old_bytes) {
        *need_out = need;
        *free_out = free_b + old_bytes;
        return 1;
      }
    }
    return 0;
  };
  size_t need = 0, free_b = 0;
  int rc = fits(c, &need, &free_b);
  if (rc < 0) return rc;
  if (rc == 1) {
    if (window_bits != 0) {
      char msg[200];
      snprintf(msg, sizeof msg, "fixed-base tables of width %u need %.1f GiB on a device with %.1f GiB free", c & 0xffu, need / 1073741824.0, free_b / 1073741824.0);
      return BP_FAIL(ctx, BP_ERR_TOO_LARGE, msg);
    }
    uint32_t pick = BP_SRS_TABLES_OFF;
    for (uint32_t cc : {22u, 24u}) {
      if (cc <= c || !srs_width_pays(cc, lead->n)) continue;
      rc = fits(cc, &need, &free_b);
      if (rc < 0) return rc;
      if (rc == 0) { pick = cc; break; }
    }
    c = pick;
  }
  // accepted (or nothing fits: the SRS ends up without tables): only now do the old tables go
  for (const SrsShard& s : sh) BP_TRY(lift(ctx, s.m, srs_precompute_one(s.m, s.e, BP_SRS_TABLES_OFF)));
  if (c == BP_SRS_TABLES_OFF) return BP_OK;
  for (const SrsShard& s : sh) BP_TRY(lift(ctx, s.m, srs_precompute_one(s.m, s.e, c)));
  return BP_OK;
}

// INTERNAL, not part of include/bp_msm_ntt.h: the memory-budget decision of bp_srs_precompute made testable without filling a
// 288-GB device (a test that hogs memory until ~400 MiB are left depends on when other processes' frees reach the
// driver).  bytes != 0: bp_srs_precompute on this context decides as if hipMemGetInfo had reported that many free bytes on every
// device (the bytes of the tables the SRS holds now still count as free on top); 0: the real reading again.  Nothing else reads it.
extern "C" int bpx_set_free_bytes_probe(bp_ctx* ctx, uint64_t bytes) {
  if (!ctx) return BP_ERR_INVALID_ARG;
  ctx->free_bytes_probe = bytes;
  return BP_OK;
}

int bp_srs_table_info(bp_ctx* ctx, uint64_t srs_handle, uint32_t* window_bits, uint32_t* windows, uint64_t* bytes) {
  if (!ctx) return BP_ERR_INVALID_ARG;
  std::vector<SrsShard> sh;
  BP_TRY(srs_shards(ctx, srs_handle, &sh));
  if (window_bits) *window_bits = sh[0].e->table_c;
  if (windows) *windows = sh[0].e->table_W;
  if (bytes) {
    *bytes = 0;
    for (const SrsShard& s : sh)
      if (s.e->d_table) *bytes += (uint64_t)s.e->table_W * s.e->n * sizeof(g1_affine28);
  }
  return BP_OK;
}

// capi_srs_check.hip -- C ABI, part 2c: the STRUCTURE of an SRS.  Are its points the powers of one tau, the tau of x_2
// (bp_srs_powers_reduce, bp_srs_check_powers)?  Do shipped Lagrange points belong to those powers (bp_srs_adopt_lagrange)?  And the
// step a ceremony repeats: a different scalar for every point (bp_srs_scale; bp_g2_mul for x_2).  The checks are random linear
// combinations: MSMs over ranges of the resident SRS through the path every commitment takes (bp_msm_g1_partial: srs_shards,
// msm_launch / msm_finish, tables included) against ONE vector rho^i made on the device, a host pairing check (pairing_host.hpp), and
// the prefix search of srs_check_host.hpp when a check fails.  The one kernel of its own is srs_scale (srs_kernels.hpp).
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "ctx.hpp"
#include "pairing_host.hpp"
#include "srs_check_host.hpp"

#include "capi_common.hpp"

using namespace bp;

// rho of a check: canonical, and neither 0 (the sum would look at one element) nor 1 (errors could cancel)
static int rho_in(bp_ctx* ctx, const void* rho32, int fmt, fr_t* rho) {
  if (!fr_from_bytes(*rho, (const uint8_t*)rho32, fmt)) return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, "rho >= q");
  if (big_eq(*rho, Fr::zero()) || big_eq(*rho, Fr::one())) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "rho must be at least 2 (and drawn with 128 bits of entropy)");
  return BP_OK;
}
// *d_v = rho^0 .. rho^(n-1), Montgomery, in a workspace of the context: fr_scale_powers_run over ones, enqueued on ctx->stream
static int rho_powers(bp_ctx* ctx, const fr_t& rho, size_t n, fr_t** d_v) {
  fr_t* d_ones;
  BP_TRY(ws_get(ctx, "srs.check_ones", std::max<size_t>(n, 1) * sizeof(fr_t), (void**)&d_ones));
  BP_TRY(ws_get(ctx, "srs.check_v", std::max<size_t>(n, 1) * sizeof(fr_t), (void**)d_v));
  if (n == 0) return BP_OK;
  BP_HIP(ctx, hipMemsetAsync(d_ones, 0, n * sizeof(fr_t), ctx->stream));
  BP_TRY(fr_scalar_run(ctx, d_ones, Fr::one(), d_ones, n, 0));
  return fr_scale_powers_run(ctx, d_ones, n, rho, *d_v);
}
// sum_{i < n} d_scalars[i] P_{first+i}: the range MSM of every commitment, scalars on the context's primary device
static int range_msm(bp_ctx* ctx, uint64_t srs, size_t first, const fr_t* d_scalars, size_t n, g1_proj* out) {
  uint8_t part[144];
  BP_TRY(bp_msm_g1_partial(ctx, srs, first, d_scalars, n, BP_FR_MONT, 1, part));
  memcpy(out, part, 144);
  return BP_OK;
}
// (A, B) over the pairs [first, first + n_pairs) against d_v[0 .. n_pairs)
static int powers_reduce_run(bp_ctx* ctx, uint64_t srs, size_t first, size_t n_pairs, const fr_t* d_v, uint8_t out192[192]) {
  g1_proj A, B;
  BP_TRY(range_msm(ctx, srs, first, d_v, n_pairs, &A));
  BP_TRY(range_msm(ctx, srs, first + 1, d_v, n_pairs, &B));
  host_encode96(out192, A);
  host_encode96(out192 + 96, B);
  return BP_OK;
}
// the handle's entry on ctx, which must hold powers (a Lagrange SRS has no "next power")
static int monomial_entry(bp_ctx* ctx, uint64_t srs, const char* what, SrsEntry** e) {
  BP_TRY(srs_find(ctx, srs, e));
  if ((*e)->basis != BP_BASIS_MONOMIAL) return BP_FAIL(ctx, BP_ERR_BASIS, what);
  return BP_OK;
}

int bp_srs_powers_reduce(bp_ctx* ctx, uint64_t srs_handle, size_t first, size_t n_pairs, const void* rho32, int scalar_fmt, uint8_t out192[192]) {
  if (!ctx || !rho32 || !out192 || !fmt_ok(scalar_fmt)) return BP_ERR_INVALID_ARG;
  SrsEntry* e;
  BP_TRY(monomial_entry(ctx, srs_handle, "bp_srs_powers_reduce: a Lagrange SRS has no consecutive powers", &e));
  if (first >= e->n_global || n_pairs > e->n_global - first - 1)
    return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "bp_srs_powers_reduce: first + n_pairs + 1 exceeds the SRS's length");
  fr_t rho;
  BP_TRY(rho_in(ctx, rho32, scalar_fmt, &rho));
  if (n_pairs == 0) {
    encode_identity_pair(out192);
    return BP_OK;
  }
  DeviceGuard guard(ctx->device);
  fr_t* d_v;
  BP_TRY(rho_powers(ctx, rho, n_pairs, &d_v));
  return powers_reduce_run(ctx, srs_handle, first, n_pairs, d_v, out192);
}

// the stats of the two verdict calls: reset on entry, the wall time written when the call leaves
struct CheckClock {
  bp_ctx* ctx;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit CheckClock(bp_ctx* c) : ctx(c) {
    ctx->srs_check_reduces = ctx->srs_check_pairings = 0;
    ctx->srs_check_ms = 0;
  }
  ~CheckClock() { ctx->srs_check_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

int bp_srs_check_powers(bp_ctx* ctx, uint64_t srs_handle, const uint8_t x2_192[192], const void* rho32, int scalar_fmt, uint32_t checks,
                        size_t* first_bad) {
  if (first_bad) *first_bad = SIZE_MAX;
  if (!ctx || !x2_192 || !rho32 || !fmt_ok(scalar_fmt) || (checks & ~BP_SRS_CHECK_GENERATOR)) return BP_ERR_INVALID_ARG;
  const CheckClock clock(ctx);
  SrsEntry* e;
  BP_TRY(monomial_entry(ctx, srs_handle, "bp_srs_check_powers: a Lagrange SRS has no consecutive powers", &e));
  const size_t len = e->n_global;
  fr_t rho;
  BP_TRY(rho_in(ctx, rho32, scalar_fmt, &rho));
  g2_affine x2;
  const int rc_x2 = pairing_decode_x2(x2, x2_192, PAIRING_CHECK_G2_SUBGROUP);
  if (rc_x2 == BP_ERR_INVALID_ARG) return BP_FAIL(ctx, rc_x2, "bp_srs_check_powers: x_2 is the identity (tau = 0 is not a setup)");
  if (rc_x2 != BP_OK) return BP_FAIL(ctx, rc_x2, "bp_srs_check_powers: x_2 rejected (encoding, flags, not on the curve, or not in the subgroup)");
  if ((checks & BP_SRS_CHECK_GENERATOR) && len) {
    uint8_t p0[96], gen[96];
    BP_TRY(bp_srs_export(ctx, srs_handle, 0, 1, p0));
    host_encode96(gen, g1_from_affine(g1_affine_generator()));
    if (memcmp(p0, gen, 96) != 0) {
      if (first_bad) *first_bad = 0;
      return BP_FAIL(ctx, BP_ERR_BAD_POINT, "point 0 is not the G1 generator");
    }
  }
  if (len <= 1) return BP_OK;
  DeviceGuard guard(ctx->device);
  fr_t* d_v;
  BP_TRY(rho_powers(ctx, rho, len - 1, &d_v));
  std::vector<fp2_t> lines(PAIRING_TABLE_FP2);
  g2_prepare(lines.data(), x2);
  const fp2_t* gen_lines = g2_generator_lines();
  int err = BP_OK;
  // do the pairs [0, k) hold?  An error ends the search: every later question is answered "no" at once
  auto holds = [&](size_t k) {
    if (err != BP_OK) return false;
    uint8_t pair[192];
    ctx->srs_check_reduces++;
    err = powers_reduce_run(ctx, srs_handle, 0, k, d_v, pair);
    if (err != BP_OK) return false;
    g1_affine a, b;
    if (pairing_decode_g1(a, pair, false) || pairing_decode_g1(b, pair + 96, false)) {
      err = BP_FAIL(ctx, BP_ERR_HIP, "bp_srs_check_powers: a reduce returned a point that does not decode");
      return false;
    }
    ctx->srs_check_pairings++;
    return pairing_check_one(a, b, lines.data(), gen_lines, nullptr);
  };
  const size_t k = lowest_failing_prefix(len - 1, holds);
  if (err != BP_OK) return err;
  if (k == SIZE_MAX) return BP_OK;
  if (first_bad) *first_bad = k;             // pair k - 1 is the lowest that fails: P_k != tau P_{k-1}
  char msg[160];
  snprintf(msg, sizeof msg, "point %llu is not tau times point %llu (tau: the one of x_2)", (unsigned long long)k, (unsigned long long)(k - 1));
  return BP_FAIL(ctx, BP_ERR_BAD_POINT, msg);
}

int bp_srs_check_last_stats(bp_ctx* ctx, uint32_t* reduces, uint32_t* pairings, float* ms) {
  if (!ctx) return BP_ERR_INVALID_ARG;
  if (reduces) *reduces = ctx->srs_check_reduces;
  if (pairings) *pairings = ctx->srs_check_pairings;
  if (ms) *ms = ctx->srs_check_ms;
  return BP_OK;
}

// the shards of `src` copied device to device into new entries (srs_register) of the same ranges, tagged Lagrange over 2^log_n
static int srs_clone_lagrange(bp_ctx* ctx, uint64_t src, uint32_t log_n, uint64_t* out) {
  std::vector<SrsShard> sh;
  BP_TRY(srs_shards(ctx, src, &sh));
  std::vector<uint64_t> hs;
  int rc = BP_OK;
  for (size_t r = 0; r < sh.size() && rc == BP_OK; r++) {
    bp_ctx* m = sh[r].m;
    const SrsEntry& src_e = *sh[r].e;
    DeviceGuard member(m->device);
    g1_affine* d_pts = nullptr;
    hipError_t he = hipMalloc((void**)&d_pts, std::max<size_t>(src_e.n, 1) * sizeof(g1_affine));
    if (he == hipSuccess && src_e.n) he = hipMemcpyAsync(d_pts, src_e.d_points, src_e.n * sizeof(g1_affine), hipMemcpyDeviceToDevice, m->stream);
    if (he != hipSuccess) {
      if (d_pts) (void)hipFree(d_pts);
      rc = fail(ctx, BP_ERR_HIP, "adopt: copy of the points", he, __FILE__, __LINE__);
      break;
    }
    uint64_t h = 0;
    rc = lift(ctx, m, srs_register(m, d_pts, src_e.n, src_e.first, src_e.n_global, &h));      // waits for m's stream: the copy is done behind it
    if (rc == BP_OK) {
      SrsEntry& e = m->srs[h];
      e.basis = BP_BASIS_LAGRANGE;
      e.log_n = log_n;
      hs.push_back(h);
    }
  }
  if (rc != BP_OK) {
    for (size_t k = 0; k < hs.size(); k++) (void)srs_free_one(sh[k].m, hs[k]);
    return rc;
  }
  if (sh.size() > 1) ctx->srs[hs[0]].member_handle = hs;
  *out = hs[0];
  return BP_OK;
}

int bp_srs_adopt_lagrange(bp_ctx* ctx, uint64_t points_handle, uint64_t powers_handle, uint32_t log_n, const void* rho32, int scalar_fmt,
                          uint64_t* lagrange_handle, size_t* first_bad) {
  if (first_bad) *first_bad = SIZE_MAX;
  if (!ctx || !rho32 || !lagrange_handle || !fmt_ok(scalar_fmt)) return BP_ERR_INVALID_ARG;
  const CheckClock clock(ctx);
  SrsEntry *pts, *pow;
  BP_TRY(monomial_entry(ctx, points_handle, "bp_srs_adopt_lagrange: the points are already tagged Lagrange", &pts));
  BP_TRY(monomial_entry(ctx, powers_handle, "bp_srs_adopt_lagrange: the powers must be a powers-of-tau SRS, not a Lagrange one", &pow));
  if (log_n > 24) return BP_FAIL(ctx, BP_ERR_TOO_LARGE, "log_n > 24");
  const size_t n = (size_t)1 << log_n;
  if (pts->n_global != n) return BP_FAIL(ctx, BP_ERR_LENGTH, "bp_srs_adopt_lagrange: exactly 2^log_n points expected");
  if (pow->n_global < n) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "bp_srs_adopt_lagrange: fewer than 2^log_n powers");
  fr_t rho;
  BP_TRY(rho_in(ctx, rho32, scalar_fmt, &rho));
  DeviceGuard guard(ctx->device);
  fr_t *d_v, *d_c;
  BP_TRY(rho_powers(ctx, rho, n, &d_v));
  BP_TRY(ws_get(ctx, "srs.check_c", n * sizeof(fr_t), (void**)&d_c));
  int err = BP_OK;
  // are the points [0, k) the Lagrange points of the powers?  v zeroed from k on: sum_{i<k} v_i points_i against sum_j c_j powers_j
  auto holds = [&](size_t k) {
    if (err != BP_OK) return false;
    ctx->srs_check_reduces++;
    g1_proj lhs, rhs;
    auto step = [&]() -> int {
      BP_HIP(ctx, hipMemcpyAsync(d_c, d_v, k * sizeof(fr_t), hipMemcpyDeviceToDevice, ctx->stream));
      if (k < n) BP_HIP(ctx, hipMemsetAsync(d_c + k, 0, (n - k) * sizeof(fr_t), ctx->stream));
      if (log_n) BP_TRY(ntt_run(ctx, d_c, log_n, 1, 1, n));
      BP_TRY(range_msm(ctx, points_handle, 0, d_v, k, &lhs));
      return range_msm(ctx, powers_handle, 0, d_c, n, &rhs);
    };
    err = step();
    if (err != BP_OK) return false;
    uint8_t l96[96], r96[96];
    host_encode96(l96, lhs);
    host_encode96(r96, rhs);
    return memcmp(l96, r96, 96) == 0;
  };
  const size_t k = lowest_failing_prefix(n, holds);
  if (err != BP_OK) return err;
  if (k != SIZE_MAX) {
    if (first_bad) *first_bad = k - 1;
    char msg[160];
    snprintf(msg, sizeof msg, "point %llu is not the Lagrange point of the powers over the 2^%u-th roots of unity", (unsigned long long)(k - 1), log_n);
    return BP_FAIL(ctx, BP_ERR_BAD_POINT, msg);
  }
  return srs_clone_lagrange(ctx, points_handle, log_n, lagrange_handle);
}

// One shard of bp_srs_scale on its member m: d_proj = scalars x points, normalised into a new entry.  `scalars` is the shard's slice,
// in host memory (where 0), in HBM of m's device (1) or in HBM of src_device behind the leader's event `ready` (2).
static int srs_scale_one(bp_ctx* m, const SrsEntry& src, const uint8_t* scalars, int fmt, int where, int src_device, hipEvent_t ready,
                         hipEvent_t* ev, uint64_t* handle) {
  DeviceGuard guard(m->device);
  const size_t n = src.n;
  fr_t* d_k;
  g1_proj* d_proj;
  uint32_t* bad;
  BP_TRY(ws_get(m, "io.scalars", std::max<size_t>(n, 1) * sizeof(fr_t), (void**)&d_k));
  BP_TRY(ws_get(m, "srs.scale_proj", std::max<size_t>(n, 1) * sizeof(g1_proj), (void**)&d_proj));
  BP_TRY(fr_bad_word(m, fmt, &bad));
  if (n) {
    if (where == 0) {
      BP_HIP(m, hipMemcpyAsync(d_k, scalars, n * sizeof(fr_t), hipMemcpyHostToDevice, m->stream));
    } else {
      if (where == 2) BP_HIP(m, hipStreamWaitEvent(m->stream, ready, 0));
      if (where == 1 || !peer_path(m, src_device)) BP_HIP(m, hipMemcpyAsync(d_k, scalars, n * sizeof(fr_t), hipMemcpyDeviceToDevice, m->stream));
      else BP_HIP(m, hipMemcpyPeerAsync(d_k, m->device, scalars, src_device, n * sizeof(fr_t), m->stream));
    }
  }
  if (fmt == BP_FR_BYTES_LE) BP_TRY(fr_convert_run(m, d_k, n, 0, bad));
  g1_affine* d_pts = nullptr;
  BP_HIP(m, hipMalloc((void**)&d_pts, std::max<size_t>(n, 1) * sizeof(g1_affine)));
  int rc = BP_OK;
  uint32_t h_bad = 0;
  hipError_t he = hipEventRecord(ev[2], m->stream);
  if (he == hipSuccess) rc = srs_scale_run(m, src.d_points, d_k, n, d_proj);
  if (he == hipSuccess && rc == BP_OK) he = hipEventRecord(ev[3], m->stream);
  if (he == hipSuccess && rc == BP_OK) rc = srs_from_projective_run(m, d_proj, n, d_pts);
  if (he == hipSuccess && rc == BP_OK) he = hipEventRecord(ev[4], m->stream);
  if (he == hipSuccess && rc == BP_OK && bad) he = hipMemcpyAsync(&h_bad, bad, sizeof h_bad, hipMemcpyDeviceToHost, m->stream);
  if (he == hipSuccess && rc == BP_OK) he = stream_wait(m->stream);
  if (he != hipSuccess) rc = fail(m, BP_ERR_HIP, "bp_srs_scale", he, __FILE__, __LINE__);
  if (rc == BP_OK && h_bad) rc = BP_FAIL(m, BP_ERR_BAD_SCALAR, "bp_srs_scale: a scalar >= q");
  if (rc != BP_OK) {
    (void)stream_wait(m->stream);
    (void)hipFree(d_pts);
    return rc;
  }
  BP_TRY(srs_register(m, d_pts, n, src.first, src.n_global, handle));
  SrsEntry& e = m->srs[*handle];
  e.basis = src.basis;
  e.log_n = src.log_n;
  return BP_OK;
}

int bp_srs_scale(bp_ctx* ctx, uint64_t srs_handle, const void* scalars, size_t n, int scalar_fmt, int scalars_on_device, uint64_t* out_handle,
                 size_t* first_bad) {
  if (first_bad) *first_bad = SIZE_MAX;
  if (!ctx || !out_handle || !fmt_ok(scalar_fmt) || (n && !scalars)) return BP_ERR_INVALID_ARG;
  std::vector<SrsShard> sh;
  BP_TRY(srs_shards(ctx, srs_handle, &sh));
  if (n != sh[0].e->n_global) return BP_FAIL(ctx, BP_ERR_LENGTH, "bp_srs_scale: one scalar per point of the SRS expected");
  for (float& v : ctx->srs_scale_ms) v = 0;
  // the subgroup test, always: shards in ascending point order, so the first failing one holds the lowest index
  std::vector<hipEvent_t*> evs(sh.size());
  for (size_t r = 0; r < sh.size(); r++) {
    const SrsShard& s = sh[r];
    DeviceGuard guard(s.m->device);
    BP_TRY(lift(ctx, s.m, ev_get(s.m, "srs.scale", 5, hipEventDefault, &evs[r])));
    BP_HIP(ctx, hipEventRecord(evs[r][0], s.m->stream));
    uint64_t bad = ~0ull;
    BP_TRY(lift(ctx, s.m, srs_subgroup_run(s.m, s.e->d_points, s.e->n, &bad)));
    BP_HIP(ctx, hipEventRecord(evs[r][1], s.m->stream));
    if (bad != ~0ull) {
      if (first_bad) *first_bad = s.e->first + (size_t)(bad >> 2);
      char msg[160];
      snprintf(msg, sizeof msg, "bp_srs_scale: point %llu is not in the prime-order subgroup", (unsigned long long)(s.e->first + (bad >> 2)));
      return BP_FAIL(ctx, BP_ERR_BAD_POINT, msg);
    }
  }
  if (sh.size() > 1 && scalars_on_device) {              // the members' copies must see what the leader's stream has produced
    DeviceGuard guard(ctx->device);
    BP_HIP(ctx, hipEventRecord(ctx->ev[4], ctx->stream));
  }
  std::vector<uint64_t> hs;
  int rc = BP_OK;
  for (size_t r = 0; r < sh.size() && rc == BP_OK; r++) {
    const SrsEntry& src = *sh[r].e;
    const int where = !scalars_on_device ? 0 : (r == 0 ? 1 : 2);
    uint64_t h = 0;
    rc = lift(ctx, sh[r].m, srs_scale_one(sh[r].m, src, (const uint8_t*)scalars + src.first * sizeof(fr_t), scalar_fmt, where, ctx->device, ctx->ev[4], evs[r], &h));
    if (rc != BP_OK) break;
    hs.push_back(h);
    DeviceGuard guard(sh[r].m->device);
    float ms[3] = {0, 0, 0};
    if (hipEventElapsedTime(&ms[0], evs[r][0], evs[r][1]) != hipSuccess || hipEventElapsedTime(&ms[1], evs[r][2], evs[r][3]) != hipSuccess ||
        hipEventElapsedTime(&ms[2], evs[r][3], evs[r][4]) != hipSuccess)
      (void)hipGetLastError();
    for (int k = 0; k < 3; k++) ctx->srs_scale_ms[k] += ms[k];
  }
  if (rc != BP_OK) {
    for (size_t k = 0; k < hs.size(); k++) (void)srs_free_one(sh[k].m, hs[k]);
    return rc;
  }
  if (sh.size() > 1) ctx->srs[hs[0]].member_handle = hs;
  *out_handle = hs[0];
  return BP_OK;
}
int bp_srs_scale_last_stats(bp_ctx* ctx, float stage_ms[3]) {
  if (!ctx || !stage_ms) return BP_ERR_INVALID_ARG;
  for (int k = 0; k < 3; k++) stage_ms[k] = ctx->srs_scale_ms[k];
  return BP_OK;
}

int bp_g2_mul(const uint8_t q192[192], const uint8_t k32[32], uint8_t out192[192]) {
  if (!q192 || !k32 || !out192) return BP_ERR_INVALID_ARG;
  return host_g2_mul(q192, k32, out192);
}

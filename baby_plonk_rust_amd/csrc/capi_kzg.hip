// capi_kzg.hip -- C ABI, part 9: KZG openings in the basis of the SRS (bp_kzg_open, bp_kzg_open_device) and the reduction of m
// opening claims to the two G1 points whose pairings decide them (bp_kzg_verify_reduce).  Field kernels: kzg_kernels.hpp through
// kzg.hip; host scalars: kzg_host.hpp; the proof is one commit_many against the same SRS; decoding, the subgroup test and the MSMs of
// the reduce are the SRS loader's and msm.hip's.
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx.hpp"
#include "g1_check.hpp"
#include "kzg_host.hpp"

#include "capi_common.hpp"

using namespace bp;

constexpr size_t KZG_MAX_COUNT = 16;

// the context's five "kzg" events: [0..2] the boundaries of an opening's two stages (values + quotient | commit), [3..4] the two ends of a reduce
static int kzg_events(bp_ctx* ctx, hipEvent_t** ev) { return ev_get(ctx, "kzg", 5, hipEventDefault, ev); }

// the part both entry points share: d_polys are HBM-resident Montgomery vectors on the context's primary device
static int kzg_open_core(bp_ctx* ctx, SrsEntry* e, uint64_t srs, const fr_t* const* d_polys, const size_t* n, size_t count, int basis, const fr_t& z,
                         const fr_t* nu, fr_t* y, g1_proj* W) {
  fr_t pows[KZG_MAX_COUNT];
  kzg_powers(nu, count, pows);
  hipEvent_t* ev;
  BP_TRY(kzg_events(ctx, &ev));
  BP_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
  fr_t* d_q = nullptr;
  size_t nq = 0;
  if (basis == BP_BASIS_LAGRANGE) {
    BP_TRY(kzg_open_lagrange_run(ctx, d_polys, count, e->log_n, z, pows, y, &d_q));
    nq = e->n_global;
  } else {
    BP_TRY(kzg_open_monomial_run(ctx, d_polys, n, count, z, pows, y, &d_q, &nq));
  }
  BP_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
  *W = g1_identity();
  if (nq) {
    const fr_t* qs[1] = {d_q};
    BP_TRY(commit_many(ctx, srs, qs, &nq, 1, W));
  }
  BP_HIP(ctx, hipEventRecord(ev[2], ctx->stream));
  BP_HIP(ctx, stream_wait(ctx->stream));
  BP_HIP(ctx, hipEventElapsedTime(&ctx->kzg_ms[0], ev[0], ev[1]));
  BP_HIP(ctx, hipEventElapsedTime(&ctx->kzg_ms[1], ev[1], ev[2]));
  return BP_OK;
}

// the argument rules of both open calls; on BP_OK *e is the SRS's entry
static int kzg_open_check(bp_ctx* ctx, uint64_t srs, const void* const* polys, const size_t* n, size_t count, int basis, const void* z32,
                          const void* nu32, int fmt, void* y_out, uint8_t* w96, SrsEntry** e) {
  if (!ctx || !polys || !n || !z32 || !y_out || !w96 || !fmt_ok(fmt) || !basis_ok(basis)) return BP_ERR_INVALID_ARG;
  if (count < 1 || count > KZG_MAX_COUNT) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "kzg open: 1 to 16 polynomials in one call");
  if (!nu32 && count > 1) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "kzg open: nu may be NULL for a single polynomial only");
  for (size_t j = 0; j < count; j++)
    if (n[j] && !polys[j]) return BP_ERR_INVALID_ARG;
  const auto it = ctx->srs.find(srs);
  if (it == ctx->srs.end()) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "kzg open: unknown SRS handle");
  *e = &it->second;
  if (basis != (*e)->basis) return BP_FAIL(ctx, BP_ERR_BASIS, "kzg open: the polynomials are not in the basis of the SRS");
  for (size_t j = 0; j < count; j++) {
    if (basis == BP_BASIS_LAGRANGE && n[j] != (*e)->n_global)
      return BP_FAIL(ctx, BP_ERR_LENGTH, "kzg open: a Lagrange polynomial must have exactly srs_len values");
    if (basis == BP_BASIS_MONOMIAL && n[j] > (*e)->n_global + 1)
      return BP_FAIL(ctx, BP_ERR_LENGTH, "kzg open: the quotient has more coefficients than the SRS has points");
  }
  return BP_OK;
}

static int kzg_scalars_in(bp_ctx* ctx, const void* z32, const void* nu32, int fmt, fr_t* z, fr_t* nu) {
  if (!fr_from_bytes(*z, (const uint8_t*)z32, fmt) || (nu32 && !fr_from_bytes(*nu, (const uint8_t*)nu32, fmt)))
    return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, "kzg open: scalar >= q");
  return BP_OK;
}

static void kzg_open_out(const fr_t* y, size_t count, int fmt, const g1_proj& W, void* y_out, uint8_t* w96) {
  for (size_t j = 0; j < count; j++) fr_to_bytes((uint8_t*)y_out + 32 * j, y[j], fmt);
  host_encode96(w96, W);
}

int bp_kzg_open_device(bp_ctx* ctx, uint64_t srs_handle, const void* const* d_polys, const size_t* n, size_t count, int basis, const void* z32,
                       const void* nu32_or_null, int scalar_fmt, void* y_out, uint8_t w96[96]) {
  SrsEntry* e = nullptr;
  BP_TRY(kzg_open_check(ctx, srs_handle, d_polys, n, count, basis, z32, nu32_or_null, scalar_fmt, y_out, w96, &e));
  fr_t z, nu, y[KZG_MAX_COUNT];
  BP_TRY(kzg_scalars_in(ctx, z32, nu32_or_null, scalar_fmt, &z, &nu));
  DeviceGuard guard(ctx->device);
  g1_proj W;
  BP_TRY(kzg_open_core(ctx, e, srs_handle, reinterpret_cast<const fr_t* const*>(d_polys), n, count, basis, z, nu32_or_null ? &nu : nullptr, y, &W));
  kzg_open_out(y, count, scalar_fmt, W, y_out, w96);
  return BP_OK;
}

int bp_kzg_open(bp_ctx* ctx, uint64_t srs_handle, const void* const* polys, const size_t* n, size_t count, int basis, const void* z32,
                const void* nu32_or_null, int scalar_fmt, void* y_out, uint8_t w96[96]) {
  SrsEntry* e = nullptr;
  BP_TRY(kzg_open_check(ctx, srs_handle, polys, n, count, basis, z32, nu32_or_null, scalar_fmt, y_out, w96, &e));
  fr_t z, nu, y[KZG_MAX_COUNT];
  BP_TRY(kzg_scalars_in(ctx, z32, nu32_or_null, scalar_fmt, &z, &nu));
  DeviceGuard guard(ctx->device);
  size_t total = 0;
  for (size_t j = 0; j < count; j++) total += n[j];
  fr_t* d_in;
  uint32_t* bad;
  BP_TRY(ws_get(ctx, "kzg.in", (total ? total : 1) * sizeof(fr_t), (void**)&d_in));
  BP_TRY(fr_bad_word(ctx, scalar_fmt, &bad));
  const fr_t* ptrs[KZG_MAX_COUNT];
  size_t off = 0;
  for (size_t j = 0; j < count; j++) {
    ptrs[j] = d_in + off;
    if (n[j]) BP_HIP(ctx, hipMemcpyAsync(d_in + off, polys[j], n[j] * sizeof(fr_t), hipMemcpyHostToDevice, ctx->stream));
    off += n[j];
  }
  if (scalar_fmt == BP_FR_BYTES_LE) BP_TRY(fr_convert_run(ctx, d_in, total, 0, bad));
  g1_proj W;
  BP_TRY(kzg_open_core(ctx, e, srs_handle, ptrs, n, count, basis, z, nu32_or_null ? &nu : nullptr, y, &W));
  if (bad) {
    uint32_t h = 0;
    BP_HIP(ctx, hipMemcpyAsync(&h, bad, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    BP_HIP(ctx, stream_wait(ctx->stream));
    if (h) return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, "kzg open: a polynomial value >= q");
  }
  kzg_open_out(y, count, scalar_fmt, W, y_out, w96);
  return BP_OK;
}

// ------------------------------------------------------------------------------------------------------- the batch check
static int kzg_reduce_run(bp_ctx* ctx, const uint8_t* commitments96, size_t m, size_t count, const fr_t* sc_c, const fr_t* sc_w, const fr_t* sc_a,
                          const fr_t& sc_g, const uint8_t* proofs96, uint32_t checks, uint8_t out192[192], size_t* first_bad) {
  const size_t n_c = m * count, n_pts = n_c + m, n_all = n_pts + 1;          // C_ij row by row | W_i | G
  uint8_t* d_bytes;
  g1_affine* d_pts;
  g1_affine28* d_p28;
  fr_t* d_sc;                                                                // c_ij | w_i | g | a_i
  BP_TRY(ws_get(ctx, "kzg.v_bytes", n_pts * 96, (void**)&d_bytes));
  BP_TRY(ws_get(ctx, "kzg.v_points", n_all * sizeof(g1_affine), (void**)&d_pts));
  BP_TRY(ws_get(ctx, "kzg.v_p28", n_all * sizeof(g1_affine28), (void**)&d_p28));
  BP_TRY(ws_get(ctx, "kzg.v_scalars", (n_all + m) * sizeof(fr_t), (void**)&d_sc));
  hipEvent_t* ev;
  BP_TRY(kzg_events(ctx, &ev));
  hipStream_t st = ctx->stream;
  BP_HIP(ctx, hipEventRecord(ev[3], st));
  const g1_affine gen = g1_affine_generator();
  BP_HIP(ctx, hipMemcpyAsync(d_bytes, commitments96, n_c * 96, hipMemcpyHostToDevice, st));
  BP_HIP(ctx, hipMemcpyAsync(d_bytes + n_c * 96, proofs96, m * 96, hipMemcpyHostToDevice, st));
  BP_HIP(ctx, hipMemcpyAsync(d_pts + n_pts, &gen, sizeof gen, hipMemcpyHostToDevice, st));
  BP_HIP(ctx, hipMemcpyAsync(d_sc, sc_c, n_c * sizeof(fr_t), hipMemcpyHostToDevice, st));
  BP_HIP(ctx, hipMemcpyAsync(d_sc + n_c, sc_w, m * sizeof(fr_t), hipMemcpyHostToDevice, st));
  BP_HIP(ctx, hipMemcpyAsync(d_sc + n_pts, &sc_g, sizeof(fr_t), hipMemcpyHostToDevice, st));
  BP_HIP(ctx, hipMemcpyAsync(d_sc + n_all, sc_a, m * sizeof(fr_t), hipMemcpyHostToDevice, st));
  if (srs_decode_run(ctx, d_bytes, n_pts, d_pts) != BP_OK) {
    // the decoder says that a record was refused, not which: the rare path looks on the host, claim by claim
    g1_affine pt;
    for (size_t i = 0; i < m; i++) {
      bool ok = host_point96(pt, proofs96 + 96 * i);
      for (size_t j = 0; j < count && ok; j++) ok = host_point96(pt, commitments96 + 96 * (i * count + j));
      if (ok) continue;
      if (first_bad) *first_bad = i;
      char msg[120];
      snprintf(msg, sizeof msg, "claim %llu: a point was rejected (encoding, flags or not on the curve)", (unsigned long long)i);
      return BP_FAIL(ctx, BP_ERR_BAD_POINT, msg);
    }
    return BP_ERR_BAD_POINT;                                                 // the decoder's own message stands
  }
  if (checks & 1) {
    uint64_t bad_c = ~0ull, bad_w = ~0ull;
    BP_TRY(srs_subgroup_run(ctx, d_pts, n_c, &bad_c));
    BP_TRY(srs_subgroup_run(ctx, d_pts + n_c, m, &bad_w));
    size_t claim = SIZE_MAX;
    if (bad_c != ~0ull) claim = (size_t)(bad_c >> 2) / count;
    if (bad_w != ~0ull) claim = std::min(claim, (size_t)(bad_w >> 2));
    if (claim != SIZE_MAX) {
      if (first_bad) *first_bad = claim;
      char msg[120];
      snprintf(msg, sizeof msg, "claim %llu: a point is not in the prime-order subgroup", (unsigned long long)claim);
      return BP_FAIL(ctx, BP_ERR_BAD_POINT, msg);
    }
  }
  BP_TRY(srs_to28_into(ctx, d_pts, n_all, d_p28));
  g1_proj A, B;
  BP_TRY(msm_run(ctx, d_p28, n_all, d_sc, BP_FR_MONT, 0, 0, &B));
  BP_TRY(msm_run(ctx, d_p28 + n_c, m, d_sc + n_all, BP_FR_MONT, 0, 0, &A));
  BP_HIP(ctx, hipEventRecord(ev[4], st));
  BP_HIP(ctx, stream_wait(st));
  BP_HIP(ctx, hipEventElapsedTime(&ctx->kzg_ms[2], ev[3], ev[4]));
  host_encode96(out192, A);
  host_encode96(out192 + 96, B);
  return BP_OK;
}

int bp_kzg_verify_reduce(bp_ctx* ctx, const uint8_t* commitments96, size_t m, size_t count, const void* z, const void* y, const void* nu_or_null,
                         const uint8_t* proofs96, const void* weights_or_null, int scalar_fmt, uint32_t checks, uint8_t out192[192],
                         size_t* first_bad) {
  if (!ctx || !out192 || !fmt_ok(scalar_fmt) || (m && (!commitments96 || !z || !y || !proofs96))) return BP_ERR_INVALID_ARG;
  if (count < 1 || count > KZG_MAX_COUNT) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "bp_kzg_verify_reduce: 1 to 16 polynomials per claim");
  if (!nu_or_null && count > 1 && m) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "bp_kzg_verify_reduce: nu may be NULL for single-polynomial claims only");
  if (!weights_or_null && m > 1) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "bp_kzg_verify_reduce: weights may be NULL for a single claim only");
  if (m >= ((size_t)1 << 31) / (count + 1) - 1) return BP_FAIL(ctx, BP_ERR_TOO_LARGE, "bp_kzg_verify_reduce: m (count + 1) + 1 >= 2^31 points");
  if (first_bad) *first_bad = SIZE_MAX;
  ctx->kzg_ms[2] = 0;
  if (m == 0) {
    encode_identity_pair(out192);
    return BP_OK;
  }
  // the scalars, on the host: m (count + 2) products
  std::vector<fr_t> zs(m), ys(m * count), nus(nu_or_null ? m : 0), rs(weights_or_null ? m : 0), sc_c(m * count), sc_w(m), sc_a(m);
  const uint8_t *zb = (const uint8_t*)z, *yb = (const uint8_t*)y, *nb = (const uint8_t*)nu_or_null, *rb = (const uint8_t*)weights_or_null;
  for (size_t i = 0; i < m; i++) {
    bool ok = fr_from_bytes(zs[i], zb + 32 * i, scalar_fmt);
    for (size_t j = 0; j < count && ok; j++) ok = fr_from_bytes(ys[i * count + j], yb + 32 * (i * count + j), scalar_fmt);
    if (ok && nb) ok = fr_from_bytes(nus[i], nb + 32 * i, scalar_fmt);
    if (ok && rb) ok = fr_from_bytes(rs[i], rb + 32 * i, scalar_fmt);
    if (!ok) {
      if (first_bad) *first_bad = i;
      char msg[96];
      snprintf(msg, sizeof msg, "claim %llu: a scalar is not canonical (>= q)", (unsigned long long)i);
      return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, msg);
    }
  }
  fr_t sc_g;
  kzg_reduce_scalars(m, count, zs.data(), ys.data(), nb ? nus.data() : nullptr, rb ? rs.data() : nullptr, sc_c.data(), sc_w.data(), sc_a.data(), &sc_g);
  DeviceGuard guard(ctx->device);
  return kzg_reduce_run(ctx, commitments96, m, count, sc_c.data(), sc_w.data(), sc_a.data(), sc_g, proofs96, checks, out192, first_bad);
}

int bp_kzg_last_stats(bp_ctx* ctx, float ms[3]) {
  if (!ctx || !ms) return BP_ERR_INVALID_ARG;
  for (int k = 0; k < 3; k++) ms[k] = ctx->kzg_ms[k];
  return BP_OK;
}

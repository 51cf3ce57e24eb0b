// capi_kzg_open_all.hip -- C ABI, part 9b: all n = 2^log_n opening proofs of one polynomial on its domain (bp_kzg_open_all,
// bp_kzg_open_all_device), its n / l cell proofs on the cosets of the domain (bp_kzg_open_cosets, bp_kzg_open_cosets_device: the
// same core with log_l > 0) and the table they keep per SRS (bp_srs_open_all_prepare, bp_srs_open_cosets_prepare).  The mathematics
// and the index maps: kzg_open_all.hpp, kzg_open_cosets.hpp; the transforms over G1: srs.hip (open_all_*_run, open_cosets_*_run); the
// Fr transforms: ntt.hip.  The reduction of cell claims: capi_kzg_cells.hip.
#include <string.h>

#include <vector>

#include "ctx.hpp"
#include "g1_ntt.hpp"

#include "capi_common.hpp"

using namespace bp;

// the argument rules every entry point shares; on BP_OK *e is the SRS's entry (the leader's, for a group)
static int open_all_srs_check(bp_ctx* ctx, uint64_t srs, uint32_t log_n, SrsEntry** e) {
  BP_TRY(srs_find(ctx, srs, e));
  if ((*e)->basis != BP_BASIS_MONOMIAL) return BP_FAIL(ctx, BP_ERR_BASIS, "kzg open all: the SRS must be powers of tau, not a Lagrange SRS");
  if (log_n >= G1_NTT_MAX_LOG) return BP_FAIL(ctx, BP_ERR_TOO_LARGE, "kzg open all: log_n >= 24 (the transform of 2n points is the limit)");
  if (((size_t)1 << log_n) - 1 > (*e)->n_global) return BP_FAIL(ctx, BP_ERR_LENGTH, "kzg open all: the SRS has fewer than n - 1 points");
  return BP_OK;
}
static int open_all_poly_check(bp_ctx* ctx, const void* poly, size_t n_values, int basis, uint32_t log_n) {
  const size_t n = (size_t)1 << log_n;
  if (basis == BP_BASIS_LAGRANGE && n_values != n) return BP_FAIL(ctx, BP_ERR_LENGTH, "kzg open all: a Lagrange polynomial must have exactly n values");
  if (basis == BP_BASIS_MONOMIAL && n_values > n) return BP_FAIL(ctx, BP_ERR_LENGTH, "kzg open all: more than n coefficients");
  if (n_values && !poly) return BP_ERR_INVALID_ARG;
  return BP_OK;
}

// the table of the entry -- DFT_2n(S^), or for log_l > 0 the l transforms DFT_R(S^(j)) side by side -- built (and *built set) unless it
// is there for this key (log_n, log_l); log_l < log_n.  Waits for the stream.
static int open_all_table(bp_ctx* ctx, uint64_t srs, SrsEntry* e, uint32_t log_n, uint32_t log_l, bool* built) {
  *built = false;
  if (e->d_open_all && e->open_all_log_n == log_n && e->open_all_log_l == log_l) return BP_OK;
  const size_t n = (size_t)1 << log_n;
  const size_t used = log_l ? n - ((size_t)1 << log_l) : n - 1;      // the points the map reads: P_0 .. P_{n-l-1} (l = 1: S^ stops at P_{n-2})
  std::vector<SrsShard> sh;
  BP_TRY(srs_shards(ctx, srs, &sh, 0, used));
  const g1_affine* d_src = sh[0].e->d_points;            // a plain context: the resident points as they are
  if (sh.size() > 1) {                                   // a group: the points read to the leader, as bp_srs_lagrange collects them
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
  if (e->d_open_all) {                                   // a table for another key goes first: the peak is one table, not two
    BP_HIP(ctx, stream_wait(ctx->stream));               // (after a failed build the entry has none; the next call builds again)
    (void)hipFree(e->d_open_all);
    e->d_open_all = nullptr;
  }
  g1_affine* d_table = nullptr;
  BP_HIP(ctx, hipMalloc((void**)&d_table, 2 * n * sizeof(g1_affine)));
  const int rc = open_cosets_table_run(ctx, d_src, log_n, log_l, d_table);      // log_l = 0: open_all_table_run
  if (rc != BP_OK) {
    (void)hipFree(d_table);
    return rc;
  }
  e->d_open_all = d_table;
  e->open_all_log_n = log_n;
  e->open_all_log_l = log_l;
  *built = true;
  return BP_OK;
}

int bp_srs_open_all_prepare(bp_ctx* ctx, uint64_t srs_handle, uint32_t log_n) {
  if (!ctx) return BP_ERR_INVALID_ARG;
  SrsEntry* e = nullptr;
  BP_TRY(open_all_srs_check(ctx, srs_handle, log_n, &e));
  if (log_n == 0) return BP_OK;                          // one proof, the identity: no table
  DeviceGuard guard(ctx->device);
  ctx->g1_ntt_pass_ms.clear();
  bool built;
  return open_all_table(ctx, srs_handle, e, log_n, 0, &built);
}

// The part both entry points share, behind their checks.  d_poly: n_values Montgomery elements on the context's device.  d_values_out
// (may be null) and d_bytes_out: workspaces of the context that hold the n values (Montgomery; log_l > 0: in cell order) and the
// n / l x 96 proof bytes on return; the stream has been waited for.  log_l < log_n.
static int open_all_core(bp_ctx* ctx, uint64_t srs, SrsEntry* e, const fr_t* d_poly, size_t n_values, int basis, uint32_t log_n, uint32_t log_l,
                         bool want_values, fr_t** d_values_out, uint8_t** d_bytes_out) {
  const size_t n = (size_t)1 << log_n, r = n >> log_l;
  const uint32_t log_R = log_n - log_l + 1;
  fr_t *d_f, *d_vals, *d_sc, *d_cells = nullptr;
  g1_affine* d_pts;
  uint8_t* d_bytes;
  BP_TRY(ws_get(ctx, "kzg.oa_f", n * sizeof(fr_t), (void**)&d_f));
  BP_TRY(ws_get(ctx, "kzg.oa_values", n * sizeof(fr_t), (void**)&d_vals));
  BP_TRY(ws_get(ctx, "kzg.oa_scalars", 2 * n * sizeof(fr_t), (void**)&d_sc));
  BP_TRY(ws_get(ctx, "kzg.oa_points", n * sizeof(g1_affine), (void**)&d_pts));
  BP_TRY(ws_get(ctx, "kzg.oa_bytes", n * 96, (void**)&d_bytes));
  if (log_l && want_values) BP_TRY(ws_get(ctx, "kzg.oc_cells", n * sizeof(fr_t), (void**)&d_cells));
  hipEvent_t* ev;
  BP_TRY(ev_get(ctx, "kzg.oa", 5, hipEventDefault, &ev));
  hipStream_t st = ctx->stream;
  ctx->g1_ntt_pass_ms.clear();
  BP_HIP(ctx, hipEventRecord(ev[0], st));
  bool built;
  BP_TRY(open_all_table(ctx, srs, e, log_n, log_l, &built));
  BP_HIP(ctx, hipEventRecord(ev[1], st));
  // the field work: the twiddles of the G1 transforms where this log_n does not have them yet (so that the Toeplitz stage is its
  // passes alone), the coefficients, the values f(w^i), and N^-1 DFT_2n(c^)
  BP_TRY(log_l ? open_cosets_twiddles_run(ctx, log_n, log_l) : open_all_twiddles_run(ctx, log_n));
  const fr_t* d_coeffs = d_poly;
  size_t n_coeffs = n_values;
  if (basis == BP_BASIS_LAGRANGE) {
    BP_HIP(ctx, hipMemcpyAsync(d_f, d_poly, n * sizeof(fr_t), hipMemcpyDeviceToDevice, st));
    BP_TRY(ntt_run(ctx, d_f, log_n, 1, 1, n));
    if (want_values) BP_HIP(ctx, hipMemcpyAsync(d_vals, d_poly, n * sizeof(fr_t), hipMemcpyDeviceToDevice, st));
    d_coeffs = d_f;
    n_coeffs = n;
  } else if (want_values) {
    BP_HIP(ctx, hipMemsetAsync(d_vals, 0, n * sizeof(fr_t), st));
    if (n_values) BP_HIP(ctx, hipMemcpyAsync(d_vals, d_poly, n_values * sizeof(fr_t), hipMemcpyDeviceToDevice, st));
    BP_TRY(ntt_run(ctx, d_vals, log_n, 0, 1, n));
  }
  if (d_cells) {                                         // the values in cell order: place k l + j holds f(w^(k + r j))
    BP_TRY(open_cosets_cell_order_run(ctx, log_n, log_l, d_vals, d_cells));
    d_vals = d_cells;
  }
  const fr_t scale = finv(fr_from_u64((uint64_t)(2 * r)));      // R^-1 (N^-1 for l = 1), Montgomery: the G1 inverse transform then multiplies by nothing
  if (log_l) {
    BP_TRY(open_cosets_chat_run(ctx, log_n, log_l, d_coeffs, n_coeffs, scale, d_sc));
    const size_t l = (size_t)1 << log_l, step = 32768;   // the l columns side by side, ONE batched transform (ntt_run: < 65536 at once)
    for (size_t at = 0; at < l; at += step) BP_TRY(ntt_run(ctx, d_sc + at * 2 * r, log_R, 0, l - at < step ? l - at : step, 2 * r));
  } else {
    BP_TRY(open_all_chat_run(ctx, log_n, d_coeffs, n_coeffs, scale, d_sc));
    BP_TRY(ntt_run(ctx, d_sc, log_n + 1, 0, 1, 2 * n));
  }
  BP_HIP(ctx, hipEventRecord(ev[2], st));
  BP_TRY(open_cosets_proofs_run(ctx, e->d_open_all, d_sc, log_n, log_l, d_pts, ev[3]));      // log_l = 0: open_all_proofs_run
  BP_TRY(srs_encode_run(ctx, d_pts, r, d_bytes));
  BP_HIP(ctx, hipEventRecord(ev[4], st));
  BP_HIP(ctx, stream_wait(st));
  for (int k = 0; k < 4; k++) BP_HIP(ctx, hipEventElapsedTime(&ctx->kzg_open_all_ms[k], ev[k], ev[k + 1]));
  if (!built) ctx->kzg_open_all_ms[0] = 0;               // the table was there: what lies between the two events is the lookup
  *d_values_out = d_vals;
  *d_bytes_out = d_bytes;
  return BP_OK;
}

// log_n == 0: one proof, the identity (the quotient of a constant is zero); the value is f_0 and no kernel runs
static void open_all_single(uint8_t* proofs96) {
  memset(proofs96, 0, 96);
  proofs96[0] = 0x40;
}

int bp_kzg_open_all_device(bp_ctx* ctx, uint64_t srs_handle, const void* d_poly, size_t n_values, int basis, uint32_t log_n, void* values_mont_host,
                           uint8_t* proofs96) {
  if (!ctx || !proofs96 || !basis_ok(basis)) return BP_ERR_INVALID_ARG;
  SrsEntry* e = nullptr;
  BP_TRY(open_all_srs_check(ctx, srs_handle, log_n, &e));
  BP_TRY(open_all_poly_check(ctx, d_poly, n_values, basis, log_n));
  DeviceGuard guard(ctx->device);
  const size_t n = (size_t)1 << log_n;
  if (log_n == 0) {
    fr_t f0 = Fr::zero();
    if (n_values) {
      BP_HIP(ctx, hipMemcpyAsync(&f0, d_poly, sizeof f0, hipMemcpyDeviceToHost, ctx->stream));
      BP_HIP(ctx, stream_wait(ctx->stream));
    }
    for (int k = 0; k < 4; k++) ctx->kzg_open_all_ms[k] = 0;
    if (values_mont_host) memcpy(values_mont_host, &f0, sizeof f0);
    open_all_single(proofs96);
    return BP_OK;
  }
  fr_t* d_vals;
  uint8_t* d_bytes;
  BP_TRY(open_all_core(ctx, srs_handle, e, (const fr_t*)d_poly, n_values, basis, log_n, 0, values_mont_host != nullptr, &d_vals, &d_bytes));
  if (values_mont_host) BP_HIP(ctx, hipMemcpyAsync(values_mont_host, d_vals, n * sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream));
  BP_HIP(ctx, hipMemcpyAsync(proofs96, d_bytes, n * 96, hipMemcpyDeviceToHost, ctx->stream));
  BP_HIP(ctx, stream_wait(ctx->stream));
  return BP_OK;
}

int bp_kzg_open_all(bp_ctx* ctx, uint64_t srs_handle, const void* poly, size_t n_values, int basis, int scalar_fmt, uint32_t log_n, void* values,
                    uint8_t* proofs96) {
  if (!ctx || !proofs96 || !basis_ok(basis) || !fmt_ok(scalar_fmt)) return BP_ERR_INVALID_ARG;
  SrsEntry* e = nullptr;
  BP_TRY(open_all_srs_check(ctx, srs_handle, log_n, &e));
  BP_TRY(open_all_poly_check(ctx, poly, n_values, basis, log_n));
  const size_t n = (size_t)1 << log_n;
  if (log_n == 0) {
    fr_t f0 = Fr::zero();
    if (n_values && !fr_from_bytes(f0, (const uint8_t*)poly, scalar_fmt)) return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, "kzg open all: a polynomial value >= q");
    for (int k = 0; k < 4; k++) ctx->kzg_open_all_ms[k] = 0;
    if (values) fr_to_bytes((uint8_t*)values, f0, scalar_fmt);
    open_all_single(proofs96);
    return BP_OK;
  }
  DeviceGuard guard(ctx->device);
  StreamDrain drain{ctx->stream};                        // the upload reads the caller's pageable memory
  fr_t* d_in;
  uint32_t* bad;
  BP_TRY(fr_bad_word(ctx, scalar_fmt, &bad));
  BP_TRY(upload_fr(ctx, "kzg.oa_in", poly, n_values, n, scalar_fmt, &d_in, bad));
  if (bad) {                                             // refused before anything is computed or written
    uint32_t h = 0;
    BP_HIP(ctx, hipMemcpyAsync(&h, bad, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    BP_HIP(ctx, stream_wait(ctx->stream));
    if (h) return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, "kzg open all: a polynomial value >= q");
  }
  fr_t* d_vals;
  uint8_t* d_bytes;
  BP_TRY(open_all_core(ctx, srs_handle, e, d_in, n_values, basis, log_n, 0, values != nullptr, &d_vals, &d_bytes));
  if (values) {
    if (scalar_fmt == BP_FR_BYTES_LE) BP_TRY(fr_convert_run(ctx, d_vals, n, 1));
    BP_HIP(ctx, hipMemcpyAsync(values, d_vals, n * sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  BP_HIP(ctx, hipMemcpyAsync(proofs96, d_bytes, n * 96, hipMemcpyDeviceToHost, ctx->stream));
  BP_HIP(ctx, stream_wait(ctx->stream));
  return BP_OK;
}

// ---- cell proofs: l = 2^log_l values and ONE proof per coset (kzg_open_cosets.hpp) -----------------------------------------------------
int open_cosets_srs_check(bp_ctx* ctx, uint64_t srs, uint32_t log_n, uint32_t log_l, SrsEntry** e) {
  BP_TRY(srs_find(ctx, srs, e));
  if ((*e)->basis != BP_BASIS_MONOMIAL) return BP_FAIL(ctx, BP_ERR_BASIS, "kzg open cosets: the SRS must be powers of tau, not a Lagrange SRS");
  if (log_l > log_n) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "kzg open cosets: log_l > log_n (a cell larger than the domain)");
  if (log_n >= G1_NTT_MAX_LOG) return BP_FAIL(ctx, BP_ERR_TOO_LARGE, "kzg open cosets: log_n >= 24");
  if (((size_t)1 << log_n) - ((size_t)1 << log_l) > (*e)->n_global) return BP_FAIL(ctx, BP_ERR_LENGTH, "kzg open cosets: the SRS has fewer than n - l points");
  return BP_OK;
}

int bp_srs_open_cosets_prepare(bp_ctx* ctx, uint64_t srs_handle, uint32_t log_n, uint32_t log_l) {
  if (!ctx) return BP_ERR_INVALID_ARG;
  if (log_l == 0) return bp_srs_open_all_prepare(ctx, srs_handle, log_n);
  SrsEntry* e = nullptr;
  BP_TRY(open_cosets_srs_check(ctx, srs_handle, log_n, log_l, &e));
  if (log_l == log_n) return BP_OK;                      // one proof, the identity: no table
  DeviceGuard guard(ctx->device);
  ctx->g1_ntt_pass_ms.clear();
  bool built;
  return open_all_table(ctx, srs_handle, e, log_n, log_l, &built);
}

// l = n >= 2: one cell, the whole domain; q = f div (x^n - 1) is zero for n coefficients, the proof is the identity and no kernel over G1
// runs.  *d_values_out (when want_values): the n values on the context's device, natural order = cell order.  Enqueued, not waited for.
static int open_cosets_whole(bp_ctx* ctx, const fr_t* d_poly, size_t n_values, int basis, uint32_t log_n, bool want_values, fr_t** d_values_out) {
  const size_t n = (size_t)1 << log_n;
  for (int k = 0; k < 4; k++) ctx->kzg_open_all_ms[k] = 0;
  ctx->g1_ntt_pass_ms.clear();
  *d_values_out = nullptr;
  if (!want_values) return BP_OK;
  fr_t* d_vals;
  BP_TRY(ws_get(ctx, "kzg.oa_values", n * sizeof(fr_t), (void**)&d_vals));
  BP_HIP(ctx, hipMemsetAsync(d_vals, 0, n * sizeof(fr_t), ctx->stream));
  if (n_values) BP_HIP(ctx, hipMemcpyAsync(d_vals, d_poly, n_values * sizeof(fr_t), hipMemcpyDeviceToDevice, ctx->stream));
  if (basis == BP_BASIS_MONOMIAL && log_n) BP_TRY(ntt_run(ctx, d_vals, log_n, 0, 1, n));      // n = 1: the value is f_0
  *d_values_out = d_vals;
  return BP_OK;
}

// capi_common.hpp: the core behind the checks for coefficients that are in HBM already (bp_kzg_recover_cells hands its result over here)
int open_cosets_resident(bp_ctx* ctx, uint64_t srs, SrsEntry* e, const fr_t* d_poly, size_t n_values, uint32_t log_n, uint32_t log_l, bool want_values,
                         fr_t** d_values_out, uint8_t** d_bytes_out) {
  *d_bytes_out = nullptr;
  if (log_l == log_n) return open_cosets_whole(ctx, d_poly, n_values, BP_BASIS_MONOMIAL, log_n, want_values, d_values_out);
  return open_all_core(ctx, srs, e, d_poly, n_values, BP_BASIS_MONOMIAL, log_n, log_l, want_values, d_values_out, d_bytes_out);
}

int bp_kzg_open_cosets_device(bp_ctx* ctx, uint64_t srs_handle, const void* d_poly, size_t n_values, int basis, uint32_t log_n, uint32_t log_l,
                              void* values_mont_host, uint8_t* proofs96) {
  if (!ctx || !proofs96 || !basis_ok(basis)) return BP_ERR_INVALID_ARG;
  if (log_l == 0) return bp_kzg_open_all_device(ctx, srs_handle, d_poly, n_values, basis, log_n, values_mont_host, proofs96);
  SrsEntry* e = nullptr;
  BP_TRY(open_cosets_srs_check(ctx, srs_handle, log_n, log_l, &e));
  BP_TRY(open_all_poly_check(ctx, d_poly, n_values, basis, log_n));
  DeviceGuard guard(ctx->device);
  const size_t n = (size_t)1 << log_n, r = n >> log_l;
  fr_t* d_vals;
  uint8_t* d_bytes = nullptr;
  if (log_l == log_n) BP_TRY(open_cosets_whole(ctx, (const fr_t*)d_poly, n_values, basis, log_n, values_mont_host != nullptr, &d_vals));
  else BP_TRY(open_all_core(ctx, srs_handle, e, (const fr_t*)d_poly, n_values, basis, log_n, log_l, values_mont_host != nullptr, &d_vals, &d_bytes));
  if (values_mont_host) BP_HIP(ctx, hipMemcpyAsync(values_mont_host, d_vals, n * sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream));
  if (d_bytes) BP_HIP(ctx, hipMemcpyAsync(proofs96, d_bytes, r * 96, hipMemcpyDeviceToHost, ctx->stream));
  BP_HIP(ctx, stream_wait(ctx->stream));
  if (!d_bytes) open_all_single(proofs96);
  return BP_OK;
}

int bp_kzg_open_cosets(bp_ctx* ctx, uint64_t srs_handle, const void* poly, size_t n_values, int basis, int scalar_fmt, uint32_t log_n, uint32_t log_l,
                       void* values, uint8_t* proofs96) {
  if (!ctx || !proofs96 || !basis_ok(basis) || !fmt_ok(scalar_fmt)) return BP_ERR_INVALID_ARG;
  if (log_l == 0) return bp_kzg_open_all(ctx, srs_handle, poly, n_values, basis, scalar_fmt, log_n, values, proofs96);
  SrsEntry* e = nullptr;
  BP_TRY(open_cosets_srs_check(ctx, srs_handle, log_n, log_l, &e));
  BP_TRY(open_all_poly_check(ctx, poly, n_values, basis, log_n));
  const size_t n = (size_t)1 << log_n, r = n >> log_l;
  DeviceGuard guard(ctx->device);
  StreamDrain drain{ctx->stream};                        // the upload reads the caller's pageable memory
  fr_t* d_in;
  uint32_t* bad;
  BP_TRY(fr_bad_word(ctx, scalar_fmt, &bad));
  BP_TRY(upload_fr(ctx, "kzg.oa_in", poly, n_values, n, scalar_fmt, &d_in, bad));
  if (bad) {                                             // refused before anything is computed or written
    uint32_t h = 0;
    BP_HIP(ctx, hipMemcpyAsync(&h, bad, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    BP_HIP(ctx, stream_wait(ctx->stream));
    if (h) return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, "kzg open cosets: a polynomial value >= q");
  }
  fr_t* d_vals;
  uint8_t* d_bytes = nullptr;
  if (log_l == log_n) BP_TRY(open_cosets_whole(ctx, d_in, n_values, basis, log_n, values != nullptr, &d_vals));
  else BP_TRY(open_all_core(ctx, srs_handle, e, d_in, n_values, basis, log_n, log_l, values != nullptr, &d_vals, &d_bytes));
  if (values) {
    if (scalar_fmt == BP_FR_BYTES_LE) BP_TRY(fr_convert_run(ctx, d_vals, n, 1));
    BP_HIP(ctx, hipMemcpyAsync(values, d_vals, n * sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (d_bytes) BP_HIP(ctx, hipMemcpyAsync(proofs96, d_bytes, r * 96, hipMemcpyDeviceToHost, ctx->stream));
  BP_HIP(ctx, stream_wait(ctx->stream));
  if (!d_bytes) open_all_single(proofs96);
  return BP_OK;
}

int bp_kzg_open_all_last_stats(bp_ctx* ctx, float stage_ms[4]) {
  if (!ctx || !stage_ms) return BP_ERR_INVALID_ARG;
  for (int k = 0; k < 4; k++) stage_ms[k] = ctx->kzg_open_all_ms[k];
  return BP_OK;
}

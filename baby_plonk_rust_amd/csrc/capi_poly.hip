// capi_poly.hip -- C ABI, part 4: Polynomial and its operators (polynomial.rs:14-380), host and device-resident forms, the
// grand product and Setup::commit of a polynomial.
#include <string.h>

#include <vector>

#include "ctx.hpp"

#include "capi_common.hpp"
#include "poly_rules.hpp"

using namespace bp;
// ---------------------------------------------------------------------------------------------- Polynomial
// Every operator has a host form and a device form (HBM-resident Montgomery data).  Both ask the same rule
// of poly_rules.hpp and enqueue the same kernels: one function per operator, its two entry points only say where the vectors live.
static int poly_addsub(bp_ctx* ctx, bool device, const void* a, size_t na, const void* b, size_t nb, int basis, int fmt, void* out, size_t* n_out,
                       int op) {
  if (!ctx || !n_out || !fmt_ok(fmt) || !basis_ok(basis) || (na && !a) || (nb && !b)) return BP_ERR_INVALID_ARG;
  BP_RULE(ctx, rule_addsub(basis, na, nb, n_out));
  const size_t n = *n_out;
  if (n == 0) return BP_OK;
  if (!out) return BP_ERR_INVALID_ARG;
  DeviceGuard guard(ctx->device);
  if (device) {
    BP_TRY(fr_binary_run(ctx, (const fr_t*)a, na, (const fr_t*)b, nb, (fr_t*)out, n, op));
    BP_HIP(ctx, stream_wait(ctx->stream));
    return BP_OK;
  }
  fr_t *da, *db, *dout;
  // add/sub commute with the Montgomery map, so canonical inputs need no conversion at all
  BP_TRY(upload_fr(ctx, "io.poly_a", a, na, na, BP_FR_MONT, &da));
  BP_TRY(upload_fr(ctx, "io.poly_b", b, nb, nb, BP_FR_MONT, &db));
  BP_TRY(ws_get(ctx, "io.poly_out", n * sizeof(fr_t), (void**)&dout));
  uint32_t* bad;
  BP_TRY(fr_bad_word(ctx, fmt, &bad));                         // ... but they are still looked at
  BP_TRY(fr_flag_noncanonical_run(ctx, da, na, bad));
  BP_TRY(fr_flag_noncanonical_run(ctx, db, nb, bad));
  BP_TRY(fr_binary_run(ctx, da, na, db, nb, dout, n, op));
  return download_fr(ctx, dout, out, n, BP_FR_MONT, bad);
}
int bp_poly_add(bp_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, int basis, int scalar_fmt, void* out, size_t* n_out) {
  return poly_addsub(ctx, false, a, na, b, nb, basis, scalar_fmt, out, n_out, 0);
}
int bp_poly_sub(bp_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, int basis, int scalar_fmt, void* out, size_t* n_out) {
  return poly_addsub(ctx, false, a, na, b, nb, basis, scalar_fmt, out, n_out, 1);
}
int bp_poly_add_device(bp_ctx* ctx, const void* d_a, size_t na, const void* d_b, size_t nb, int basis, void* d_out, size_t* n_out) {
  return poly_addsub(ctx, true, d_a, na, d_b, nb, basis, BP_FR_MONT, d_out, n_out, 0);
}
int bp_poly_sub_device(bp_ctx* ctx, const void* d_a, size_t na, const void* d_b, size_t nb, int basis, void* d_out, size_t* n_out) {
  return poly_addsub(ctx, true, d_a, na, d_b, nb, basis, BP_FR_MONT, d_out, n_out, 1);
}

// Add / Sub / Mul<Scalar>; device: a and out are HBM-resident Montgomery limbs (out == a is allowed), s32 is Montgomery
static int poly_scalar_op(bp_ctx* ctx, bool device, const void* a, size_t n, int basis, const void* s32, int op, int fmt, void* out) {
  if (!ctx || !s32 || !fmt_ok(fmt) || !basis_ok(basis) || op < 0 || op > 2 || (n && (!a || !out))) return BP_ERR_INVALID_ARG;
  ScalarAction action;
  BP_RULE(ctx, rule_scalar_op(basis, op, n, &action));
  if (action == SCALAR_NOTHING) return BP_OK;
  fr_t s;
  if (device) memcpy(&s, s32, 32);
  else if (!fr_from_bytes(s, (const uint8_t*)s32, fmt)) return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, "scalar >= q");
  DeviceGuard guard(ctx->device);
  fr_t *da = (fr_t*)a, *dout = (fr_t*)out;
  uint32_t* bad = nullptr;
  if (!device) {
    BP_TRY(fr_bad_word(ctx, fmt, &bad));
    BP_TRY(upload_fr(ctx, "io.poly_a", a, n, n, fmt, &da, bad));
    BP_TRY(ws_get(ctx, "io.poly_out", n * sizeof(fr_t), (void**)&dout));
  }
  if (action == SCALAR_FIRST) {                               // copy, then values[0] += / -= rhs
    if (dout != da) BP_HIP(ctx, hipMemcpyAsync(dout, da, n * sizeof(fr_t), hipMemcpyDeviceToDevice, ctx->stream));
    BP_TRY(fr_scalar_run(ctx, da, s, dout, 1, op));
  } else {                                                    // Lagrange: += rhs for Add AND Sub (polynomial.rs:126-128)
    BP_TRY(fr_scalar_run(ctx, da, s, dout, n, action == SCALAR_MUL_ALL ? 2 : 0));
  }
  if (!device) return download_fr(ctx, dout, out, n, fmt, bad);
  BP_HIP(ctx, stream_wait(ctx->stream));
  return BP_OK;
}
int bp_poly_scalar_op(bp_ctx* ctx, const void* a, size_t n, int basis, const void* s32, int op, int scalar_fmt, void* out) {
  return poly_scalar_op(ctx, false, a, n, basis, s32, op, scalar_fmt, out);
}
int bp_poly_scalar_op_device(bp_ctx* ctx, const void* d_a, size_t n, int basis, const void* s32_mont, int op, void* d_out) {
  return poly_scalar_op(ctx, true, d_a, n, basis, s32_mont, op, BP_FR_MONT, d_out);
}

// Mul<Polynomial>; `kind` says where a, b and out live: hipMemcpyHostToDevice for host memory in format fmt (the host form),
// hipMemcpyDeviceToDevice for HBM-resident Montgomery limbs (the device form, fmt = BP_FR_MONT)
static int poly_mul(bp_ctx* ctx, hipMemcpyKind kind, const void* a, size_t na, const void* b, size_t nb, int basis, int fmt, void* out,
                    size_t* n_out) {
  if (!ctx || !n_out || !fmt_ok(fmt) || !basis_ok(basis) || !a || !b || !out) return BP_ERR_INVALID_ARG;
  uint32_t k, *bad;
  size_t N, target;
  BP_RULE(ctx, rule_mul(basis, na, nb, &k, &N, &target));
  DeviceGuard guard(ctx->device);
  fr_t* d;
  BP_TRY(ws_get(ctx, "io.poly_mul", 2 * N * sizeof(fr_t), (void**)&d));
  BP_HIP(ctx, hipMemsetAsync(d, 0, 2 * N * sizeof(fr_t), ctx->stream));
  BP_HIP(ctx, hipMemcpyAsync(d, a, na * sizeof(fr_t), kind, ctx->stream));
  BP_HIP(ctx, hipMemcpyAsync(d + N, b, nb * sizeof(fr_t), kind, ctx->stream));
  BP_TRY(fr_bad_word(ctx, fmt, &bad));
  if (fmt == BP_FR_BYTES_LE) BP_TRY(fr_convert_run(ctx, d, 2 * N, 0, bad));
  BP_TRY(ntt_run(ctx, d, k, 0, 2, N));                        // evaluate both at the N roots (polynomial.rs:255-260)
  BP_TRY(fr_binary_run(ctx, d, N, d + N, N, d, N, 2));        // pointwise product (:262-266)
  BP_TRY(ntt_run(ctx, d, k, 1, 1, N));                        // i_ntt_381 (:270)
  if (kind == hipMemcpyHostToDevice) {
    *n_out = target;                                          // [0 ..= n+m] (:272)
    return download_fr(ctx, d, out, target, fmt, bad);
  }
  BP_HIP(ctx, hipMemcpyAsync(out, d, target * sizeof(fr_t), hipMemcpyDeviceToDevice, ctx->stream));
  BP_HIP(ctx, stream_wait(ctx->stream));
  *n_out = target;
  return BP_OK;
}
int bp_poly_mul(bp_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, int basis, int scalar_fmt, void* out, size_t* n_out) {
  return poly_mul(ctx, hipMemcpyHostToDevice, a, na, b, nb, basis, scalar_fmt, out, n_out);
}
int bp_poly_mul_device(bp_ctx* ctx, const void* d_a, size_t na, const void* d_b, size_t nb, int basis, void* d_out, size_t* n_out) {
  return poly_mul(ctx, hipMemcpyDeviceToDevice, d_a, na, d_b, nb, basis, BP_FR_MONT, d_out, n_out);
}

// Div first finds its shape: the lengths with trailing zeros trimmed (polynomial.rs:325-339), whether the divisor is the binomial
// b0 + b_lead x^(nb_eff-1), and those two (Montgomery).  The host form reads it off the host data, the device form measures it.
int bp_poly_div(bp_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, int basis, int scalar_fmt, void* out, size_t* n_out) {
  if (!ctx || !n_out || !fmt_ok(scalar_fmt) || !basis_ok(basis) || (na && !a) || (nb && !b)) return BP_ERR_INVALID_ARG;
  BP_RULE(ctx, rule_div_basis(basis));
  const fr_t *ha = (const fr_t*)a, *hb = (const fr_t*)b;
  size_t na_eff, nb_eff, nq;
  fr_t b0, b_lead;
  for (na_eff = na; na_eff > 0 && big_is_zero(ha[na_eff - 1]);) na_eff--;      // zero is all-zero in both formats
  for (nb_eff = nb; nb_eff > 0 && big_is_zero(hb[nb_eff - 1]);) nb_eff--;
  BP_RULE(ctx, rule_div(na_eff, nb_eff, &nq));
  *n_out = 0;
  if (nq == 0) return BP_OK;
  if (!out) return BP_ERR_INVALID_ARG;
  DeviceGuard guard(ctx->device);
  fr_t *da, *db, *dq;
  uint32_t* bad;
  BP_TRY(fr_bad_word(ctx, scalar_fmt, &bad));
  BP_TRY(upload_fr(ctx, "io.poly_a", a, na_eff, na_eff, scalar_fmt, &da, bad));
  BP_TRY(upload_fr(ctx, "io.poly_b", b, nb_eff, nb_eff, scalar_fmt, &db, bad));
  if (!fr_from_bytes(b0, (const uint8_t*)&hb[0], scalar_fmt) || !fr_from_bytes(b_lead, (const uint8_t*)&hb[nb_eff - 1], scalar_fmt))
    return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, "scalar >= q");
  bool binomial = nb_eff >= 2;
  for (size_t i = 1; i + 1 < nb_eff && binomial; i++) binomial = big_is_zero(hb[i]);
  BP_TRY(ws_get(ctx, "io.poly_out", nq * sizeof(fr_t), (void**)&dq));
  BP_TRY(poly_div_run(ctx, da, na_eff, db, nb_eff, b0, b_lead, binomial, dq, nq));
  std::vector<fr_t> q(nq);
  BP_TRY(download_fr(ctx, dq, q.data(), nq, scalar_fmt, bad));
  // The reference inserts one quotient coefficient per loop turn and pops every newly zero leading remainder
  // term (polynomial.rs:371-376): its result is the true quotient with the zero coefficients squeezed out.
  for (size_t i = 0; i < nq; i++)
    if (!big_is_zero(q[i])) ((fr_t*)out)[(*n_out)++] = q[i];
  return BP_OK;
}
int bp_poly_div_device(bp_ctx* ctx, const void* d_a, size_t na, const void* d_b, size_t nb, int basis, void* d_out, size_t* n_out) {
  if (!ctx || !n_out || !basis_ok(basis) || (na && !d_a) || (nb && !d_b)) return BP_ERR_INVALID_ARG;
  BP_RULE(ctx, rule_div_basis(basis));
  DeviceGuard guard(ctx->device);
  const fr_t* b = (const fr_t*)d_b;
  size_t na_eff, nb_eff, nq, dummy, mid_nonzero = 0;
  fr_t b0, b_lead;
  BP_TRY(fr_nonzero_stats_run(ctx, (const fr_t*)d_a, na, 0, 0, &na_eff, &dummy));
  BP_TRY(fr_nonzero_stats_run(ctx, b, nb, 0, 0, &nb_eff, &dummy));
  BP_RULE(ctx, rule_div(na_eff, nb_eff, &nq));
  *n_out = 0;
  if (nq == 0) return BP_OK;
  if (!d_out) return BP_ERR_INVALID_ARG;
  if (nb_eff > 2) BP_TRY(fr_nonzero_stats_run(ctx, b, nb_eff, 1, nb_eff - 1, &dummy, &mid_nonzero));
  const bool binomial = nb_eff >= 2 && mid_nonzero == 0;
  BP_HIP(ctx, hipMemcpyAsync(&b0, b, sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream));
  BP_HIP(ctx, hipMemcpyAsync(&b_lead, b + (nb_eff - 1), sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream));
  BP_HIP(ctx, stream_wait(ctx->stream));
  fr_t *work, *q;
  BP_TRY(ws_get(ctx, "io.poly_div_work", na_eff * sizeof(fr_t), (void**)&work));     // the general path clobbers its dividend
  BP_HIP(ctx, hipMemcpyAsync(work, d_a, na_eff * sizeof(fr_t), hipMemcpyDeviceToDevice, ctx->stream));
  BP_TRY(ws_get(ctx, "io.poly_out", nq * sizeof(fr_t), (void**)&q));
  BP_TRY(poly_div_run(ctx, work, na_eff, b, nb_eff, b0, b_lead, binomial, q, nq));
  size_t m = nq;
  BP_TRY(fr_squeeze_zeros_run(ctx, q, &m));                   // polynomial.rs:371-376
  if (m) BP_HIP(ctx, hipMemcpyAsync(d_out, q, m * sizeof(fr_t), hipMemcpyDeviceToDevice, ctx->stream));
  BP_HIP(ctx, stream_wait(ctx->stream));
  *n_out = m;
  return BP_OK;
}

int bp_poly_evaluate(bp_ctx* ctx, const void* coeffs, size_t n, int basis, const void* x32, int scalar_fmt, void* out32) {
  if (!ctx || !x32 || !out32 || !fmt_ok(scalar_fmt) || !basis_ok(basis) || (n && !coeffs)) return BP_ERR_INVALID_ARG;
  BP_RULE(ctx, rule_evaluate(basis));
  fr_t x, r;
  if (!fr_from_bytes(x, (const uint8_t*)x32, scalar_fmt)) return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, "scalar >= q");
  DeviceGuard guard(ctx->device);
  fr_t* d;
  uint32_t* bad;
  BP_TRY(fr_bad_word(ctx, scalar_fmt, &bad));
  BP_TRY(upload_fr(ctx, "io.poly_a", coeffs, n, n, scalar_fmt, &d, bad));
  BP_TRY(poly_eval_run(ctx, d, n, x, &r, n ? bad : nullptr));
  fr_to_bytes((uint8_t*)out32, r, scalar_fmt);
  return BP_OK;
}
int bp_poly_evaluate_device(bp_ctx* ctx, const void* d_coeffs, size_t n, int basis, const void* x32_mont, void* out32_mont) {
  if (!ctx || !x32_mont || !out32_mont || !basis_ok(basis) || (n && !d_coeffs)) return BP_ERR_INVALID_ARG;
  BP_RULE(ctx, rule_evaluate(basis));
  fr_t x, r;
  memcpy(&x, x32_mont, 32);
  DeviceGuard guard(ctx->device);
  BP_TRY(poly_eval_run(ctx, (const fr_t*)d_coeffs, n, x, &r));
  memcpy(out32_mont, &r, 32);
  return BP_OK;
}
int bp_poly_last_stats(bp_ctx* ctx, uint32_t* div_path, uint64_t* chunks, uint32_t* segments) {
  if (!ctx) return BP_ERR_INVALID_ARG;
  if (div_path) *div_path = ctx->poly_div_path;
  if (chunks) *chunks = ctx->poly_div_chunks;
  if (segments) *segments = ctx->poly_div_segments;
  return BP_OK;
}
int bp_poly_scale_powers_device(bp_ctx* ctx, const void* d_a, size_t n, const void* w32_mont, void* d_out) {
  if (!ctx || !w32_mont || (n && (!d_a || !d_out))) return BP_ERR_INVALID_ARG;
  fr_t w;
  memcpy(&w, w32_mont, 32);
  DeviceGuard guard(ctx->device);
  BP_TRY(fr_scale_powers_run(ctx, (const fr_t*)d_a, n, w, (fr_t*)d_out));
  BP_HIP(ctx, stream_wait(ctx->stream));
  return BP_OK;
}
int bp_grand_product_device(bp_ctx* ctx, const void* a, const void* b, const void* c, const void* s1, const void* s2, const void* s3, size_t n,
                            const void* beta32, const void* gamma32, const void* k1_32, const void* k2_32, void* d_z) {
  if (!ctx || !beta32 || !gamma32 || !k1_32 || !k2_32 || (n && (!a || !b || !c || !s1 || !s2 || !s3 || !d_z))) return BP_ERR_INVALID_ARG;
  if (n == 0) return BP_OK;
  BP_RULE(ctx, rule_grand_product(n));
  fr_t beta, gamma, k1, k2, root;
  memcpy(&beta, beta32, 32); memcpy(&gamma, gamma32, 32); memcpy(&k1, k1_32, 32); memcpy(&k2, k2_32, 32);
  host_root_of_unity(root, n);
  DeviceGuard guard(ctx->device);
  BP_TRY(grand_product_run(ctx, (const fr_t*)a, (const fr_t*)b, (const fr_t*)c, (const fr_t*)s1, (const fr_t*)s2, (const fr_t*)s3, n, beta, gamma,
                           k1, k2, root, (fr_t*)d_z));
  BP_HIP(ctx, stream_wait(ctx->stream));
  return BP_OK;
}
// the commit rule of the SRS `srs_handle` names (rule_commit_srs); a handle the context does not know is the MSM's to refuse
static PolyRule commit_rule(bp_ctx* ctx, uint64_t srs_handle, int basis, size_t n) {
  const auto it = ctx->srs.find(srs_handle);
  if (it == ctx->srs.end()) return rule_commit(basis);
  return rule_commit_srs(basis, n, it->second.basis, it->second.n_global);
}
int bp_commit_device(bp_ctx* ctx, uint64_t srs_handle, const void* d_coeffs, size_t n, int basis, uint8_t out96[96]) {
  if (!ctx || !basis_ok(basis) || !out96) return BP_ERR_INVALID_ARG;
  BP_RULE(ctx, commit_rule(ctx, srs_handle, basis, n));
  uint8_t part[144];
  BP_TRY(bp_msm_g1_partial(ctx, srs_handle, 0, d_coeffs, n, BP_FR_MONT, 1, part));
  return bp_g1_partial_to_bytes96(part, out96);
}

// Several commitments against one SRS in one call (the three of prover.rs:249-251, of :483-485, the two of :640-641): their
// pipelines are in flight together (commit_many: per-device lanes, or queued shards on a group context), so one commitment's
// latency-bound tail runs under another's bulk kernel.
int bp_commit_many_device(bp_ctx* ctx, uint64_t srs_handle, const void* const* d_coeffs, const size_t* n, size_t count, int basis,
                          uint8_t* out96) {
  if (!ctx || !basis_ok(basis) || (count && (!d_coeffs || !n || !out96))) return BP_ERR_INVALID_ARG;
  BP_RULE(ctx, commit_rule(ctx, srs_handle, basis, count ? n[0] : 0));
  for (size_t i = 1; i < count; i++) BP_RULE(ctx, commit_rule(ctx, srs_handle, basis, n[i]));
  if (count > 64) return BP_FAIL(ctx, BP_ERR_TOO_LARGE, "more than 64 commitments in one call");
  for (size_t i = 0; i < count; i++)
    if (n[i] && !d_coeffs[i]) return BP_ERR_INVALID_ARG;
  std::vector<g1_proj> cm(count);
  BP_TRY(commit_many(ctx, srs_handle, reinterpret_cast<const fr_t* const*>(d_coeffs), n, (int)count, cm.data()));
  for (size_t i = 0; i < count; i++) host_encode96(out96 + 96 * i, cm[i]);
  return BP_OK;
}

int bp_grand_product(bp_ctx* ctx, const void* a, const void* b, const void* c, const void* s1, const void* s2, const void* s3, size_t n,
                     const void* beta32, const void* gamma32, const void* k1_32, const void* k2_32, int scalar_fmt, void* z_out) {
  if (!ctx || !fmt_ok(scalar_fmt) || !beta32 || !gamma32 || !k1_32 || !k2_32 || (n && (!a || !b || !c || !s1 || !s2 || !s3 || !z_out)))
    return BP_ERR_INVALID_ARG;
  if (n == 0) return BP_OK;
  BP_RULE(ctx, rule_grand_product(n));
  fr_t beta, gamma, k1, k2, root;
  if (!fr_from_bytes(beta, (const uint8_t*)beta32, scalar_fmt) || !fr_from_bytes(gamma, (const uint8_t*)gamma32, scalar_fmt) ||
      !fr_from_bytes(k1, (const uint8_t*)k1_32, scalar_fmt) || !fr_from_bytes(k2, (const uint8_t*)k2_32, scalar_fmt))
    return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, "scalar >= q");
  host_root_of_unity(root, n);                                   // roots_of_unity(group_order), utils.rs:45-52
  DeviceGuard guard(ctx->device);
  fr_t* cols;
  BP_TRY(ws_get(ctx, "io.gp_cols", 7 * n * sizeof(fr_t), (void**)&cols));
  const void* src[6] = {a, b, c, s1, s2, s3};
  for (int j = 0; j < 6; j++) BP_HIP(ctx, hipMemcpyAsync(cols + (size_t)j * n, src[j], n * sizeof(fr_t), hipMemcpyHostToDevice, ctx->stream));
  uint32_t* bad;
  BP_TRY(fr_bad_word(ctx, scalar_fmt, &bad));
  if (scalar_fmt == BP_FR_BYTES_LE) BP_TRY(fr_convert_run(ctx, cols, 6 * n, 0, bad));
  fr_t* z = cols + 6 * n;
  BP_TRY(grand_product_run(ctx, cols, cols + n, cols + 2 * n, cols + 3 * n, cols + 4 * n, cols + 5 * n, n, beta, gamma, k1, k2, root, z, nullptr,
                           bad));
  return download_fr(ctx, z, z_out, n, scalar_fmt);
}

int bp_commit(bp_ctx* ctx, uint64_t srs_handle, const void* coeffs, size_t n, int basis, int scalar_fmt, uint8_t out96[96]) {
  if (!ctx || !basis_ok(basis)) return BP_ERR_INVALID_ARG;
  BP_RULE(ctx, commit_rule(ctx, srs_handle, basis, n));
  return bp_msm_g1(ctx, srs_handle, coeffs, n, scalar_fmt, out96);
}


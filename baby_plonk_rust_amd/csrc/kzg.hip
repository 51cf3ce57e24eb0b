// kzg.hip -- host drivers of a KZG opening's field work (kzg_kernels.hpp): the values at the point and the quotient, in the basis
// the polynomials are held in.  Everything runs on ctx->stream; the commitment to the quotient is the caller's (capi_kzg.hip).
#include <string.h>

#include <algorithm>

#include "ctx.hpp"
#include "host_codec.hpp"
#include "kzg_host.hpp"
#include "kzg_kernels.hpp"

namespace bp {

static KzgCols kzg_cols(const fr_t* const* d_polys, const size_t* n, size_t n_all, size_t count, const fr_t* nu_pows) {
  KzgCols a;
  memset(&a, 0, sizeof a);
  a.count = (uint32_t)count;
  for (size_t j = 0; j < count; j++) {
    a.c[j] = d_polys[j];
    a.n[j] = n ? n[j] : n_all;
    a.w[j] = nu_pows[j];
  }
  return a;
}

// Lagrange form.  The shared inverses 1 / (z - w^i) come from the exclusive prefix and suffix products of fr_scan_mul_run and ONE
// host inversion of the total (~3 products per element and no inversion on the device, against ~48 per element
// for a Fermat inversion per lane of eight).
int kzg_open_lagrange_run(bp_ctx* ctx, const fr_t* const* d_polys, size_t count, uint32_t log_n, const fr_t& z, const fr_t* nu_pows,
                          fr_t* host_y, fr_t** d_q) {
  const size_t n = (size_t)1 << log_n;
  uint64_t m64 = 0;
  const bool on_domain = kzg_domain_index(z, log_n, &m64);
  const size_t m = on_domain ? (size_t)m64 : KZG_NO_INDEX;
  const unsigned blocks = (unsigned)((n + 255) / 256), sum_blocks = std::min<unsigned>(blocks, KZG_SUM_BLOCKS);
  fr_t *roots, *den, *pre, *suf, *winv, *q, *partial, *small;
  BP_TRY(ws_get(ctx, "kzg.roots", n * sizeof(fr_t), (void**)&roots));
  BP_TRY(ws_get(ctx, "kzg.den", n * sizeof(fr_t), (void**)&den));
  BP_TRY(ws_get(ctx, "kzg.pre", n * sizeof(fr_t), (void**)&pre));
  BP_TRY(ws_get(ctx, "kzg.suf", n * sizeof(fr_t), (void**)&suf));
  BP_TRY(ws_get(ctx, "kzg.winv", n * sizeof(fr_t), (void**)&winv));
  BP_TRY(ws_get(ctx, "kzg.q", n * sizeof(fr_t), (void**)&q));
  BP_TRY(ws_get(ctx, "kzg.partial", (size_t)KZG_MAX_POLYS * KZG_SUM_BLOCKS * sizeof(fr_t), (void**)&partial));
  BP_TRY(ws_get(ctx, "kzg.small", (KZG_MAX_POLYS + 2) * sizeof(fr_t), (void**)&small));      // count results, then the two scan totals
  hipStream_t st = ctx->stream;
  if (ctx->kzg_roots_ptr != roots || ctx->kzg_roots_log_n != log_n) {      // the domain's points stay resident between openings of one size
    fr_t w;
    host_root_of_unity(w, n);
    ctx->kzg_roots_ptr = nullptr;
    BP_TRY(roots_run(ctx, w, n, roots));
    ctx->kzg_roots_ptr = roots;
    ctx->kzg_roots_log_n = log_n;
  }
  const KzgCols a = kzg_cols(d_polys, nullptr, n, count, nu_pows);
  fr_t* inv = den;                                                        // the denominators are dead once they are scanned
  hipLaunchKernelGGL(kzg_lag_denoms, dim3(blocks), dim3(256), 0, st, roots, n, z, m, den);
  BP_HIP(ctx, hipGetLastError());
  BP_TRY(fr_scan_mul_run(ctx, den, n, 0, 0, pre, small + KZG_MAX_POLYS));
  BP_TRY(fr_scan_mul_run(ctx, den, n, 1, 0, suf, small + KZG_MAX_POLYS + 1));
  fr_t total, total_inv;
  BP_HIP(ctx, hipMemcpyAsync(&total, small + KZG_MAX_POLYS, sizeof(fr_t), hipMemcpyDeviceToHost, st));
  BP_HIP(ctx, stream_wait(st));
  if (big_is_zero(total)) return BP_FAIL(ctx, BP_ERR_DIV_ZERO, "kzg open: a denominator z - w^i is zero");      // cannot happen: the zero one was replaced
  fr_invert(total_inv, total);
  hipLaunchKernelGGL(kzg_lag_invert, dim3(blocks), dim3(256), 0, st, pre, suf, roots, total_inv, n, inv, winv);
  BP_HIP(ctx, hipGetLastError());
  if (on_domain) {
    hipLaunchKernelGGL(kzg_gather_row, dim3(1), dim3(256), 0, st, a, m, small);
  } else {
    hipLaunchKernelGGL(kzg_lag_values_partial, dim3(sum_blocks, (unsigned)count), dim3(256), 0, st, a, winv, n, partial);
    hipLaunchKernelGGL(kzg_sum_rows, dim3((unsigned)count), dim3(256), 0, st, partial, sum_blocks, 0, small);
  }
  BP_HIP(ctx, hipGetLastError());
  BP_HIP(ctx, hipMemcpyAsync(host_y, small, count * sizeof(fr_t), hipMemcpyDeviceToHost, st));
  BP_HIP(ctx, stream_wait(st));
  if (!on_domain) {
    const fr_t scale = kzg_barycentric_scale(z, log_n);
    for (size_t j = 0; j < count; j++) Fr::mul(host_y[j], host_y[j], scale);
  }
  const fr_t y_g = kzg_combine(nu_pows, host_y, count);
  hipLaunchKernelGGL(kzg_lag_quotient, dim3(blocks), dim3(256), 0, st, a, y_g, inv, n, m, q);
  if (on_domain) {
    hipLaunchKernelGGL(kzg_lag_diag_partial, dim3(sum_blocks), dim3(256), 0, st, q, roots, n, m, partial);
    hipLaunchKernelGGL(kzg_sum_rows, dim3(1), dim3(256), 0, st, partial, sum_blocks, 1, q + m);
  }
  BP_HIP(ctx, hipGetLastError());
  *d_q = q;
  return BP_OK;
}

// Monomial form: the values through poly_eval_many_run (eight at a time), the quotient of g = sum_j nu^j f_j by x - z through
// poly_div_run's binomial path, which never reads g_0: the remainder g(z) need not be subtracted first, and no zero coefficient
// is squeezed out.
int kzg_open_monomial_run(bp_ctx* ctx, const fr_t* const* d_polys, const size_t* n, size_t count, const fr_t& z, const fr_t* nu_pows,
                          fr_t* host_y, fr_t** d_q, size_t* nq) {
  for (size_t base = 0; base < count; base += 8) {
    const int k = (int)std::min<size_t>(8, count - base);
    fr_t x[8];
    for (int j = 0; j < k; j++) x[j] = z;
    BP_TRY(poly_eval_many_run(ctx, k, d_polys + base, n + base, x, host_y + base));
  }
  size_t len = 0;
  for (size_t j = 0; j < count; j++) len = std::max(len, n[j]);
  *d_q = nullptr;
  *nq = len ? len - 1 : 0;
  if (*nq == 0) return BP_OK;
  fr_t *g, *q;
  BP_TRY(ws_get(ctx, "kzg.g", len * sizeof(fr_t), (void**)&g));
  BP_TRY(ws_get(ctx, "kzg.q", *nq * sizeof(fr_t), (void**)&q));
  const KzgCols a = kzg_cols(d_polys, n, 0, count, nu_pows);
  hipLaunchKernelGGL(kzg_lincomb, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, ctx->stream, a, len, g);
  BP_HIP(ctx, hipGetLastError());
  fr_t b0;
  Fr::neg(b0, z);
  BP_TRY(poly_div_run(ctx, g, len, nullptr, 2, b0, Fr::one(), true, q, *nq));
  *d_q = q;
  return BP_OK;
}

// d_out[t] = - sum_i d_rho[i] d_w[i]^t d_c[i l + t], t < l (kzg_kernels.hpp: kzg_cells_combine); enqueued, not waited for
int kzg_cells_combine_run(bp_ctx* ctx, const fr_t* d_c, const fr_t* d_w, const fr_t* d_rho, size_t m, uint32_t log_l, fr_t* d_out) {
  const size_t l = (size_t)1 << log_l;
  hipLaunchKernelGGL(kzg_cells_combine, dim3((unsigned)((l + 255) / 256)), dim3(256), 0, ctx->stream, d_c, d_w, d_rho, m, log_l, d_out);
  BP_HIP(ctx, hipGetLastError());
  return BP_OK;
}

}  // namespace bp

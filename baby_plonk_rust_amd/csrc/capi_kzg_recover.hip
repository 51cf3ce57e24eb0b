// capi_kzg_recover.hip -- C ABI, part 9d: a polynomial rebuilt from m of its r = n / l cells (bp_kzg_recover, bp_kzg_recover_device) and,
// from there, all r cells and cell proofs (bp_kzg_recover_cells: the recovery, then the core of bp_kzg_open_cosets_device on the
// coefficients where they lie, in HBM).  The map and the plan: kzg_recover.hpp; the kernels: kzg_recover_kernels.hpp; the transforms,
// the powers of the shift and the scans of the batched inversion: ntt.hip, poly.hip.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ctx.hpp"
#include "kzg_recover_kernels.hpp"

#include "capi_common.hpp"

using namespace bp;

namespace {

struct RecoverCall {
  uint32_t log_n = 0, log_l = 0;
  size_t m = 0, d = 0, n_missing = 0;
  std::vector<int32_t> slot;
  std::vector<uint32_t> missing;
};

// the plan of the call, on the host; a refusal names its position in *first_bad
int recover_call(bp_ctx* ctx, uint32_t log_n, uint32_t log_l, const uint32_t* cell_index, size_t m, size_t d, RecoverCall* c, size_t* first_bad) {
  if (first_bad) *first_bad = SIZE_MAX;
  if (recover_shape_ok(log_n, log_l)) {
    c->slot.resize((size_t)1 << (log_n - log_l));
    c->missing.resize(c->slot.size());
  }
  const RecoverPlan plan = recover_plan(cell_index, m, log_n, log_l, d, c->slot.data(), c->missing.data());
  if (plan.err != BP_OK) {
    char msg[160];
    if (plan.bad != RECOVER_NO_POSITION) {
      if (first_bad) *first_bad = (size_t)plan.bad;
      snprintf(msg, sizeof msg, "kzg recover: cell index %u at position %llu is not below n / l, or is given twice", cell_index[plan.bad],
               (unsigned long long)plan.bad);
    } else if (plan.err == BP_ERR_LENGTH) {
      snprintf(msg, sizeof msg, "kzg recover: n_coeffs must be in 1 .. min(m l, n)");
    } else {
      snprintf(msg, sizeof msg, "kzg recover: log_l > log_n, log_n >= 24 or more than 2^16 cells");
    }
    return BP_FAIL(ctx, plan.err, msg);
  }
  c->log_n = log_n;
  c->log_l = log_l;
  c->m = m;
  c->d = d;
  c->n_missing = (size_t)plan.n_missing;
  return BP_OK;
}

hipEvent_t* recover_events(bp_ctx* ctx) {
  hipEvent_t* ev = nullptr;
  return ev_get(ctx, "kzg.rc", 5, hipEventDefault, &ev) == BP_OK ? ev : nullptr;
}

// Steps 1 to 4 of kzg_recover.hpp.  d_v: the m l values, Montgomery, on the context's device; d_work: n elements there, apart from d_v.
// On BP_OK d_work holds the coefficients (places d .. n - 1 are zero) and the stream has been waited for; BP_ERR_ASSERT: the cells
// agree with no polynomial of degree < d, *first_bad is the lowest non-zero index and d_work holds the interpolant.
int recover_core(bp_ctx* ctx, const RecoverCall& c, const fr_t* d_v, fr_t* d_work, size_t* first_bad) {
  const uint32_t log_n = c.log_n, log_l = c.log_l, log_r = log_n - log_l;
  const size_t n = (size_t)1 << log_n, r = (size_t)1 << log_r;
  hipStream_t st = ctx->stream;
  for (int k = 0; k < 4; k++) ctx->kzg_recover_ms[k] = 0;
  hipEvent_t* ev = recover_events(ctx);
  if (!ev) return BP_ERR_HIP;
  int32_t* d_slot;
  unsigned long long* d_low;
  BP_TRY(ws_get(ctx, "kzg.rc_slot", r * sizeof(int32_t), (void**)&d_slot));
  BP_TRY(ws_get(ctx, "kzg.rc_low", 16, (void**)&d_low));
  StreamDrain drain{st};                                 // the uploads read the plan's pageable memory
  BP_HIP(ctx, hipMemcpyAsync(d_slot, c.slot.data(), r * sizeof(int32_t), hipMemcpyHostToDevice, st));
  BP_HIP(ctx, hipEventRecord(ev[0], st));
  fr_t* d_z = nullptr;                                   // Z_dom | Z_cos
  if (c.n_missing) {
    const uint32_t n_missing = (uint32_t)c.n_missing, groups = recover_slice_groups(c.n_missing);
    fr_t *d_dom, *d_roots, *d_partial;
    uint32_t* d_missing;
    BP_TRY(ws_get(ctx, "kzg.rc_dom", r * sizeof(fr_t), (void**)&d_dom));
    BP_TRY(ws_get(ctx, "kzg.rc_missing", c.n_missing * sizeof(uint32_t), (void**)&d_missing));
    BP_TRY(ws_get(ctx, "kzg.rc_roots", c.n_missing * sizeof(fr_t), (void**)&d_roots));
    BP_TRY(ws_get(ctx, "kzg.rc_z", 2 * r * sizeof(fr_t), (void**)&d_z));
    d_partial = d_z;                                     // one group: its products ARE the evaluations
    if (groups > 1) BP_TRY(ws_get(ctx, "kzg.rc_partial", 2 * (size_t)groups * r * sizeof(fr_t), (void**)&d_partial));
    fr_t omega_r;
    (void)host_root_of_unity(omega_r, r);
    BP_TRY(roots_run(ctx, omega_r, r, d_dom));
    BP_HIP(ctx, hipMemcpyAsync(d_missing, c.missing.data(), c.n_missing * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(recover_missing_roots, dim3((n_missing + 255) / 256), dim3(256), 0, st, d_dom, d_missing, n_missing, d_roots);
    hipLaunchKernelGGL(recover_vanishing_eval, dim3((unsigned)((r + RECOVER_POINTS - 1) / RECOVER_POINTS), 2, groups), dim3(256), 0, st, d_dom,
                       (uint32_t)r, recover_coset_base(log_l), d_roots, n_missing, d_partial);
    if (groups > 1)
      hipLaunchKernelGGL(recover_vanishing_combine, dim3((unsigned)((r + 255) / 256), 2), dim3(256), 0, st, d_partial, (uint32_t)r, groups, d_z);
    BP_HIP(ctx, hipGetLastError());
  }
  BP_HIP(ctx, hipEventRecord(ev[1], st));
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(recover_spread, dim3(blocks), dim3(256), 0, st, log_n, log_l, d_slot, d_v, d_z, d_work);
  BP_HIP(ctx, hipGetLastError());
  if (log_n) BP_TRY(ntt_run(ctx, d_work, log_n, 1, 1, n));
  BP_HIP(ctx, hipEventRecord(ev[2], st));
  if (c.n_missing) {
    // (f Z)(s omega^i) / Z(s omega^i): the r inverses from the prefix and suffix products of Z_cos and ONE host inversion, as kzg.hip
    fr_t *d_tmp, *d_pre, *d_suf, *d_total;
    BP_TRY(ws_get(ctx, "kzg.rc_tmp", n * sizeof(fr_t), (void**)&d_tmp));
    BP_TRY(ws_get(ctx, "kzg.rc_pre", r * sizeof(fr_t), (void**)&d_pre));
    BP_TRY(ws_get(ctx, "kzg.rc_suf", r * sizeof(fr_t), (void**)&d_suf));
    BP_TRY(ws_get(ctx, "kzg.rc_total", 2 * sizeof(fr_t), (void**)&d_total));
    const fr_t s = fr_from_u64(KZG_RECOVER_SHIFT);
    BP_TRY(fr_scale_powers_run(ctx, d_work, n, s, d_tmp));
    if (log_n) BP_TRY(ntt_run(ctx, d_tmp, log_n, 0, 1, n));
    BP_TRY(fr_scan_mul_run(ctx, d_z + r, r, 0, 0, d_pre, d_total));
    BP_TRY(fr_scan_mul_run(ctx, d_z + r, r, 1, 0, d_suf, d_total + 1));
    fr_t total;
    BP_HIP(ctx, hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, st));
    BP_HIP(ctx, stream_wait(st));
    if (big_is_zero(total)) return BP_FAIL(ctx, BP_ERR_DIV_ZERO, "kzg recover: the vanishing polynomial is zero on the shifted domain");      // cannot happen: s^n != 1
    BP_TRY(fr_binary_run(ctx, d_pre, r, d_suf, r, d_pre, r, 2));
    BP_TRY(fr_scalar_run(ctx, d_pre, finv(total), d_pre, r, 2));
    hipLaunchKernelGGL(recover_divide, dim3(blocks), dim3(256), 0, st, log_n, log_r, d_pre, d_tmp);
    BP_HIP(ctx, hipGetLastError());
    if (log_n) BP_TRY(ntt_run(ctx, d_tmp, log_n, 1, 1, n));
    BP_TRY(fr_scale_powers_run(ctx, d_tmp, n, finv(s), d_work));
  }
  BP_HIP(ctx, hipEventRecord(ev[3], st));
  unsigned long long lowest = ~0ull;
  BP_HIP(ctx, hipMemsetAsync(d_low, 0xff, sizeof lowest, st));
  if (c.d < n) {
    hipLaunchKernelGGL(recover_high_nonzero, dim3((unsigned)((n - c.d + 255) / 256)), dim3(256), 0, st, d_work, c.d, n, d_low);
    BP_HIP(ctx, hipGetLastError());
  }
  BP_HIP(ctx, hipMemcpyAsync(&lowest, d_low, sizeof lowest, hipMemcpyDeviceToHost, st));
  BP_HIP(ctx, stream_wait(st));
  if (lowest != ~0ull) {
    if (first_bad) *first_bad = (size_t)lowest;
    char msg[160];
    snprintf(msg, sizeof msg, "kzg recover: the cells agree with no polynomial of %llu coefficients (coefficient %llu of their interpolant is not zero)",
             (unsigned long long)c.d, lowest);
    return BP_FAIL(ctx, BP_ERR_ASSERT, msg);
  }
  return BP_OK;
}

// behind the output of a call that recover_core accepted: the end of the last stage and the four times
int recover_times(bp_ctx* ctx, bool any_missing) {
  hipEvent_t* ev = recover_events(ctx);
  if (!ev) return BP_ERR_HIP;
  BP_HIP(ctx, hipEventRecord(ev[4], ctx->stream));
  BP_HIP(ctx, stream_wait(ctx->stream));
  for (int k = 0; k < 4; k++) BP_HIP(ctx, hipEventElapsedTime(&ctx->kzg_recover_ms[k], ev[k], ev[k + 1]));
  if (!any_missing) ctx->kzg_recover_ms[0] = ctx->kzg_recover_ms[2] = 0;      // steps 1 and 3 did not run: what lies between the events is nothing
  return BP_OK;
}

// the m l host values in scalar_fmt -> Montgomery in workspace "kzg.rc_in"; a canonical-bytes value >= q: the cell's position
int recover_upload(bp_ctx* ctx, const RecoverCall& c, const void* values, int fmt, fr_t** d_v, size_t* first_bad) {
  const size_t l = (size_t)1 << c.log_l, count = c.m * l;
  uint32_t* bad;
  BP_TRY(fr_bad_word(ctx, fmt, &bad));
  BP_TRY(upload_fr(ctx, "kzg.rc_in", values, count, count, fmt, d_v, bad));
  if (!bad) return BP_OK;
  uint32_t h = 0;
  BP_HIP(ctx, hipMemcpyAsync(&h, bad, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  BP_HIP(ctx, stream_wait(ctx->stream));
  if (!h) return BP_OK;
  // the device says that a value was refused, not which: the rare path looks on the host, cell by cell
  const uint8_t* vb = (const uint8_t*)values;
  for (size_t i = 0; i < count; i++) {
    if (fr_is_canonical(vb + 32 * i)) continue;
    if (first_bad) *first_bad = i >> c.log_l;
    char msg[96];
    snprintf(msg, sizeof msg, "kzg recover: cell %llu has a value that is not canonical (>= q)", (unsigned long long)(i >> c.log_l));
    return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, msg);
  }
  return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, "kzg recover: a value >= q");
}

}  // namespace

int bp_kzg_recover_device(bp_ctx* ctx, uint32_t log_n, uint32_t log_l, const uint32_t* cell_index, const void* d_values, size_t m, size_t n_coeffs,
                          void* d_coeffs, size_t* first_bad) {
  if (!ctx || !d_coeffs || (m && (!cell_index || !d_values))) return BP_ERR_INVALID_ARG;
  RecoverCall c;
  BP_TRY(recover_call(ctx, log_n, log_l, cell_index, m, n_coeffs, &c, first_bad));
  DeviceGuard guard(ctx->device);
  BP_TRY(recover_core(ctx, c, (const fr_t*)d_values, (fr_t*)d_coeffs, first_bad));
  return recover_times(ctx, c.n_missing != 0);
}

int bp_kzg_recover(bp_ctx* ctx, uint32_t log_n, uint32_t log_l, const uint32_t* cell_index, const void* values, size_t m, size_t n_coeffs,
                   int scalar_fmt, void* coeffs_out, size_t* first_bad) {
  if (!ctx || !coeffs_out || !fmt_ok(scalar_fmt) || (m && (!cell_index || !values))) return BP_ERR_INVALID_ARG;
  RecoverCall c;
  BP_TRY(recover_call(ctx, log_n, log_l, cell_index, m, n_coeffs, &c, first_bad));
  DeviceGuard guard(ctx->device);
  StreamDrain drain{ctx->stream};                        // the upload reads the caller's pageable memory
  fr_t *d_v, *d_work;
  BP_TRY(recover_upload(ctx, c, values, scalar_fmt, &d_v, first_bad));
  BP_TRY(ws_get(ctx, "kzg.rc_work", ((size_t)1 << log_n) * sizeof(fr_t), (void**)&d_work));
  BP_TRY(recover_core(ctx, c, d_v, d_work, first_bad));
  if (scalar_fmt == BP_FR_BYTES_LE) BP_TRY(fr_convert_run(ctx, d_work, n_coeffs, 1));
  BP_HIP(ctx, hipMemcpyAsync(coeffs_out, d_work, n_coeffs * sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream));
  return recover_times(ctx, c.n_missing != 0);
}

int bp_kzg_recover_cells(bp_ctx* ctx, uint64_t srs_handle, uint32_t log_n, uint32_t log_l, const uint32_t* cell_index, const void* values, size_t m,
                         size_t n_coeffs, int scalar_fmt, void* values_out, uint8_t* proofs96, size_t* first_bad) {
  if (!ctx || !proofs96 || !fmt_ok(scalar_fmt) || (m && (!cell_index || !values))) return BP_ERR_INVALID_ARG;
  RecoverCall c;
  BP_TRY(recover_call(ctx, log_n, log_l, cell_index, m, n_coeffs, &c, first_bad));
  SrsEntry* e = nullptr;
  BP_TRY(open_cosets_srs_check(ctx, srs_handle, log_n, log_l, &e));
  DeviceGuard guard(ctx->device);
  StreamDrain drain{ctx->stream};                        // the upload reads the caller's pageable memory
  const size_t n = (size_t)1 << log_n, r = n >> log_l;
  fr_t *d_v, *d_work, *d_cells = nullptr;
  uint8_t* d_bytes = nullptr;
  BP_TRY(recover_upload(ctx, c, values, scalar_fmt, &d_v, first_bad));
  BP_TRY(ws_get(ctx, "kzg.rc_work", n * sizeof(fr_t), (void**)&d_work));
  BP_TRY(recover_core(ctx, c, d_v, d_work, first_bad));
  BP_TRY(recover_times(ctx, c.n_missing != 0));
  // the second half: the coefficients stay where they are
  BP_TRY(open_cosets_resident(ctx, srs_handle, e, d_work, n_coeffs, log_n, log_l, values_out != nullptr, &d_cells, &d_bytes));
  if (values_out) {
    if (scalar_fmt == BP_FR_BYTES_LE) BP_TRY(fr_convert_run(ctx, d_cells, n, 1));
    BP_HIP(ctx, hipMemcpyAsync(values_out, d_cells, n * sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (d_bytes) BP_HIP(ctx, hipMemcpyAsync(proofs96, d_bytes, r * 96, hipMemcpyDeviceToHost, ctx->stream));
  BP_HIP(ctx, stream_wait(ctx->stream));
  if (!d_bytes) {                                        // one cell: the quotient is zero, the proof the identity
    memset(proofs96, 0, 96);
    proofs96[0] = 0x40;
  }
  return BP_OK;
}

int bp_kzg_recover_last_stats(bp_ctx* ctx, float stage_ms[4]) {
  if (!ctx || !stage_ms) return BP_ERR_INVALID_ARG;
  for (int k = 0; k < 4; k++) stage_ms[k] = ctx->kzg_recover_ms[k];
  return BP_OK;
}

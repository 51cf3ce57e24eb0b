// capi_wires.hip -- C ABI, part 5c: a circuit from its wire ids and a witness from a value per variable (bp_circuit_load_wires,
// bp_circuit_export_columns, bp_circuit_assign_device, bp_prove_assignment).  Rules: wire_plan.hpp; kernels: wire_kernels.hpp.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ctx.hpp"
#include "wire_kernels.hpp"

#include "capi_common.hpp"

using namespace bp;

namespace {

// device memory of one call: freed however the call is left
struct DevTmp {
  std::vector<void*> held;
  ~DevTmp() {
    for (void* p : held) (void)hipFree(p);
  }
  hipError_t get(size_t bytes, void** out) {
    const hipError_t e = hipMalloc(out, bytes ? bytes : 1);
    if (e == hipSuccess) held.push_back(*out);
    return e;
  }
  void* release(void* p) {      // the caller keeps p
    for (void*& h : held)
      if (h == p) h = nullptr;
    return p;
  }
};

// the stable sort of (id, cell) by id, plan.passes passes of 8 bits.  *keys / *idx: where the sorted order stands afterwards
// (no pass: the ids themselves and nullptr, the identity).
int wire_sort_run(bp_ctx* ctx, const WirePlan& plan, const uint32_t* d_ids, DevTmp& tmp, const uint32_t** keys, const uint32_t** idx) {
  *keys = d_ids;
  *idx = nullptr;
  if (plan.passes == 0) return BP_OK;
  uint32_t *k[2], *i[2], *hist, *sums;
  for (int s = 0; s < 2; s++) {
    BP_HIP(ctx, tmp.get(plan.key_bytes, (void**)&k[s]));
    BP_HIP(ctx, tmp.get(plan.key_bytes, (void**)&i[s]));
  }
  BP_HIP(ctx, tmp.get(plan.hist_bytes, (void**)&hist));
  BP_HIP(ctx, tmp.get(plan.sums_bytes, (void**)&sums));
  for (uint32_t pass = 0; pass < plan.passes; pass++) {
    uint32_t *k_out = k[pass & 1], *i_out = i[pass & 1];
    hipLaunchKernelGGL(wire_hist, dim3(plan.tiles), dim3(WIRE_BLOCK), 0, ctx->stream, *keys, plan.cells, pass, plan.tiles, hist);
    hipLaunchKernelGGL(wire_scan_chunks, dim3(plan.scan_chunks), dim3(WIRE_BLOCK), 0, ctx->stream, hist, plan.hist_entries, sums);
    hipLaunchKernelGGL(wire_scan_sums, dim3(1), dim3(WIRE_BLOCK), 0, ctx->stream, sums, plan.scan_chunks);
    hipLaunchKernelGGL(wire_scatter, dim3(plan.tiles), dim3(WIRE_BLOCK), 0, ctx->stream, *keys, *idx, plan.cells, pass, plan.tiles,
                       (const uint32_t*)hist, (const uint32_t*)sums, k_out, i_out);
    BP_HIP(ctx, hipGetLastError());
    *keys = k_out;
    *idx = i_out;
  }
  return BP_OK;
}

// a b c PI (d_pi may be null) of `cir` from a value per variable, into device memory of the caller's; waits for the stream
int wire_gather_run(bp_ctx* ctx, const CircuitEntry& cir, const void* values, size_t n_values, int scalar_fmt, int values_on_device, fr_t* d_a,
                    fr_t* d_b, fr_t* d_c, fr_t* d_pi) {
  const size_t n = (size_t)1 << cir.log_n;
  const fr_t* d_values = (const fr_t*)values;
  uint32_t* d_bad = nullptr;
  if (!values_on_device) {
    fr_t* up;
    BP_TRY(fr_bad_word(ctx, scalar_fmt, &d_bad));
    BP_TRY(upload_fr(ctx, "wires.values", values, n_values, 1, scalar_fmt, &up, d_bad));
    d_values = up;
  }
  unsigned long long* status;
  BP_TRY(ws_get(ctx, "wires.status", 16, (void**)&status));
  BP_HIP(ctx, hipMemsetAsync(status, 0xff, 8, ctx->stream));
  hipLaunchKernelGGL(wire_gather, dim3(wire_ceil_div(n, WIRE_BLOCK)), dim3(WIRE_BLOCK), 0, ctx->stream, (const uint32_t*)cir.wire_ids, n,
                     cir.n_public, d_values, n_values, d_a, d_b, d_c, d_pi, status);
  BP_HIP(ctx, hipGetLastError());
  unsigned long long worst = ~0ull;
  uint32_t bad = 0;
  BP_HIP(ctx, hipMemcpyAsync(&worst, status, sizeof worst, hipMemcpyDeviceToHost, ctx->stream));
  if (d_bad) BP_HIP(ctx, hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
  BP_HIP(ctx, stream_wait(ctx->stream));
  if (bad) return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, "assignment value >= q");
  if (worst != ~0ull) {
    char msg[200];
    snprintf(msg, sizeof msg, "assignment: %zu values do not cover the wire id of cell %llu (row %llu, column %c), the lowest such cell", n_values,
             worst, worst / 3, "ABC"[worst % 3]);
    return BP_FAIL(ctx, BP_ERR_LENGTH, msg);
  }
  return BP_OK;
}

int wires_circuit(bp_ctx* ctx, uint64_t handle, CircuitEntry** out) {
  auto it = ctx->circuits.find(handle);
  if (it == ctx->circuits.end()) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "unknown circuit handle");
  if (!it->second.wire_ids) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "the circuit was loaded from columns (bp_circuit_load): it holds no wire ids");
  *out = &it->second;
  return BP_OK;
}

}  // namespace

int bp_circuit_load_wires(bp_ctx* ctx, uint32_t log_n, const void* const selectors[5], const uint32_t* wire_ids, size_t n_public, int scalar_fmt,
                          int inputs_on_device, uint64_t* handle) {
  if (!ctx || !selectors || !wire_ids || !handle || !fmt_ok(scalar_fmt)) return BP_ERR_INVALID_ARG;
  if (log_n < 3 || log_n > WIRE_MAX_LOG_N) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "circuit: log_n must be in 3..24");
  const size_t n = (size_t)1 << log_n, cells = 3 * n;
  if (n_public > n) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "circuit: more public rows than rows");
  if (inputs_on_device && scalar_fmt != BP_FR_MONT) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "device selectors must be Montgomery");
  for (int k = 0; k < 5; k++)
    if (!selectors[k]) return BP_ERR_INVALID_ARG;
  DeviceGuard guard(ctx->device);
  hipEvent_t* ev;
  BP_TRY(ev_get(ctx, "wires", 6, hipEventDefault, &ev));
  DevTmp tmp;                       // declared before the entry: what the entry owns on success is released from it
  fr_t *lag, *roots;
  uint32_t *ids, *target, *d_max, *d_bad;
  BP_HIP(ctx, tmp.get(8 * n * sizeof(fr_t), (void**)&lag));
  BP_HIP(ctx, tmp.get(cells * sizeof(uint32_t), (void**)&ids));
  BP_HIP(ctx, tmp.get(cells * sizeof(uint32_t), (void**)&target));
  BP_HIP(ctx, tmp.get(n * sizeof(fr_t), (void**)&roots));
  BP_TRY(ws_get(ctx, "wires.status", 16, (void**)&d_max));
  const hipMemcpyKind kind = inputs_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  // stage 0: the inputs where the kernels read them
  BP_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
  for (int k = 0; k < 5; k++) BP_HIP(ctx, hipMemcpyAsync(lag + (size_t)k * n, selectors[k], n * sizeof(fr_t), kind, ctx->stream));
  BP_HIP(ctx, hipMemcpyAsync(ids, wire_ids, cells * sizeof(uint32_t), kind, ctx->stream));
  BP_TRY(fr_bad_word(ctx, scalar_fmt, &d_bad));
  if (scalar_fmt == BP_FR_BYTES_LE) BP_TRY(fr_convert_run(ctx, lag, 5 * n, 0, d_bad));
  // stage 1: the largest id and the one read-back the pass count needs
  BP_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
  BP_HIP(ctx, hipMemsetAsync(d_max, 0, sizeof(uint32_t), ctx->stream));
  hipLaunchKernelGGL(wire_max_id, dim3(wire_ceil_div(cells, WIRE_BLOCK)), dim3(WIRE_BLOCK), 0, ctx->stream, (const uint32_t*)ids, cells, d_max);
  BP_HIP(ctx, hipGetLastError());
  uint32_t max_id = 0, bad = 0;
  BP_HIP(ctx, hipMemcpyAsync(&max_id, d_max, sizeof max_id, hipMemcpyDeviceToHost, ctx->stream));
  if (d_bad) BP_HIP(ctx, hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
  BP_HIP(ctx, stream_wait(ctx->stream));
  if (bad) return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, "selector value >= q");
  const WirePlan plan = wire_plan(log_n, max_id);
  if (!wire_plan_valid(plan)) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "circuit: no valid sort plan");
  // stage 2: cells grouped by id, row-major inside a group
  BP_HIP(ctx, hipEventRecord(ev[2], ctx->stream));
  const uint32_t *keys, *idx;
  BP_TRY(wire_sort_run(ctx, plan, ids, tmp, &keys, &idx));
  // stage 3: the table of roots, then S1 S2 S3 and the cell map in one pass
  BP_HIP(ctx, hipEventRecord(ev[3], ctx->stream));
  fr_t w;
  (void)host_root_of_unity(w, (uint64_t)n);
  BP_TRY(roots_run(ctx, w, n, roots));
  hipLaunchKernelGGL(wire_link, dim3(plan.cell_blocks), dim3(WIRE_BLOCK), 0, ctx->stream, keys, idx, cells, (const fr_t*)roots, log_n, lag + 5 * n, target);
  BP_HIP(ctx, hipGetLastError());
  // stage 4: the forms every circuit handle holds
  BP_HIP(ctx, hipEventRecord(ev[4], ctx->stream));
  CircuitEntry e;
  BP_TRY(circuit_build(ctx, log_n, lag, &e));                 // waits for the stream; owns lag from here
  tmp.release(lag);
  e.sigma_target = (uint32_t*)tmp.release(target);            // the link pass wrote a permutation: bp_circuit_check_* never decode
  const uint64_t clean[4] = {0, ~0ull, 0, ~0ull};             // no finding of either kind, no position: what a decode of these columns reports
  memcpy(e.sigma_report, clean, sizeof clean);
  e.wire_ids = (uint32_t*)tmp.release(ids);
  e.n_public = n_public;
  auto finish = [&]() -> int {
    BP_HIP(ctx, hipEventRecord(ev[5], ctx->stream));
    BP_TRY(circuit_split_build(ctx, e));      // round 3 by coset over the members of a group (nothing otherwise)
    BP_HIP(ctx, stream_wait(ctx->stream));
    for (int s = 0; s < 5; s++) BP_HIP(ctx, hipEventElapsedTime(&ctx->wires_ms[s], ev[s], ev[s + 1]));
    return BP_OK;
  };
  const int rc = finish();
  if (rc != BP_OK) {
    circuit_release(e);
    return rc;
  }
  *handle = ctx->next_handle++;
  ctx->circuits[*handle] = e;
  return BP_OK;
}

int bp_circuit_load_wires_last_stats(bp_ctx* ctx, float stage_ms[5]) {
  if (!ctx || !stage_ms) return BP_ERR_INVALID_ARG;
  memcpy(stage_ms, ctx->wires_ms, 5 * sizeof(float));
  return BP_OK;
}

int bp_circuit_export_columns(bp_ctx* ctx, uint64_t circuit_handle, int scalar_fmt, void* const columns[8]) {
  if (!ctx || !columns || !fmt_ok(scalar_fmt)) return BP_ERR_INVALID_ARG;
  auto it = ctx->circuits.find(circuit_handle);
  if (it == ctx->circuits.end()) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "unknown circuit handle");
  const CircuitEntry& e = it->second;
  const size_t n = (size_t)1 << e.log_n;
  DeviceGuard guard(ctx->device);
  StreamDrain drain{ctx->stream};
  fr_t* out = nullptr;
  if (scalar_fmt == BP_FR_BYTES_LE) BP_TRY(ws_get(ctx, "wires.export", n * sizeof(fr_t), (void**)&out));
  for (int k = 0; k < 8; k++) {
    if (!columns[k]) continue;
    const fr_t* src = e.lag + (size_t)k * n;
    if (out) {                    // the handle's columns stay Montgomery: converted in a copy
      BP_HIP(ctx, hipMemcpyAsync(out, src, n * sizeof(fr_t), hipMemcpyDeviceToDevice, ctx->stream));
      BP_TRY(fr_convert_run(ctx, out, n, 1));
      src = out;
    }
    BP_HIP(ctx, hipMemcpyAsync(columns[k], src, n * sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  BP_HIP(ctx, stream_wait(ctx->stream));
  return BP_OK;
}

int bp_circuit_assign_device(bp_ctx* ctx, uint64_t circuit_handle, const void* values, size_t n_values, int scalar_fmt, int values_on_device,
                             void* d_a, void* d_b, void* d_c, void* d_pi) {
  if (!ctx || (!values && n_values) || !d_a || !d_b || !d_c || !fmt_ok(scalar_fmt)) return BP_ERR_INVALID_ARG;
  if (values_on_device && scalar_fmt != BP_FR_MONT) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "device values must be Montgomery");
  CircuitEntry* cir;
  BP_TRY(wires_circuit(ctx, circuit_handle, &cir));
  DeviceGuard guard(ctx->device);
  return wire_gather_run(ctx, *cir, values, n_values, scalar_fmt, values_on_device, (fr_t*)d_a, (fr_t*)d_b, (fr_t*)d_c, (fr_t*)d_pi);
}

int bp_prove_assignment(bp_ctx* ctx, uint64_t srs_handle, uint64_t circuit_handle, const void* values, size_t n_values, int scalar_fmt,
                        int values_on_device, const uint8_t blinders[352], uint8_t proof[624]) {
  if (!ctx || (!values && n_values) || !blinders || !proof || !fmt_ok(scalar_fmt)) return BP_ERR_INVALID_ARG;
  if (values_on_device && scalar_fmt != BP_FR_MONT) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "device values must be Montgomery");
  CircuitEntry* cir;
  BP_TRY(wires_circuit(ctx, circuit_handle, &cir));
  SrsEntry* srs;
  BP_TRY(srs_find(ctx, srs_handle, &srs));
  (void)srs;
  fr_t blind[11];
  for (int j = 0; j < 11; j++)
    if (!fr_from_bytes(blind[j], blinders + 32 * j, BP_FR_BYTES_LE)) return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, "blinder >= q");
  DeviceGuard guard(ctx->device);
  const size_t n = (size_t)1 << cir->log_n;
  fr_t* wit;
  BP_TRY(ws_get(ctx, "prove.witness", 4 * n * sizeof(fr_t), (void**)&wit));
  BP_TRY(wire_gather_run(ctx, *cir, values, n_values, scalar_fmt, values_on_device, wit, wit + n, wit + 2 * n, wit + 3 * n));
  return prove_run(ctx, srs_handle, *cir, wit, blind, proof, cir->n_public == 0);
}

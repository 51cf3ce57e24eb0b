// capi_check.hip -- C ABI, part 5b: where a witness fails its circuit (bp_circuit_check_sigma, bp_circuit_check_witness).
#include <stdio.h>
#include <string.h>

#include "ctx.hpp"
#include "witness_check_kernels.hpp"

#include "capi_common.hpp"

using namespace bp;

namespace {

// the context's six "check" events: [0..1] around the sigma decode, [2..3] around upload + conversion, [4..5] around the check kernel
int check_events(bp_ctx* ctx, hipEvent_t** ev) { return ev_get(ctx, "check", 6, hipEventDefault, ev); }

dim3 blocks_of(size_t lanes) { return dim3((unsigned)((lanes + 255) / 256)); }

// four status words on the stream: counters 0, positions ~0 (witness_check_kernels.hpp)
int status_begin(bp_ctx* ctx, unsigned long long** status) {
  BP_TRY(ws_get(ctx, "check.status", 32, (void**)status));
  BP_HIP(ctx, hipMemsetAsync(*status, 0, 16, ctx->stream));
  BP_HIP(ctx, hipMemsetAsync(*status + 2, 0xff, 16, ctx->stream));
  return BP_OK;
}

// The circuit's sigma decoded and judged, once: e.sigma_target and e.sigma_report.  *decode_ms: HIP-event time of the decode and the
// in-degree passes, 0 when the circuit already had them.  Waits for the stream when it decodes.
int sigma_ensure(bp_ctx* ctx, CircuitEntry& e, hipEvent_t ev0, hipEvent_t ev1, float* decode_ms) {
  *decode_ms = 0;
  if (e.sigma_target) return BP_OK;
  const size_t n = (size_t)1 << e.log_n, cells = 3 * n;
  SigmaConsts k;
  SigmaTable tbl;
  sigma_consts(e.log_n, &k, &tbl);
  fr_t* d_winv;
  uint32_t* d_count;
  unsigned long long* status;
  BP_TRY(ws_get(ctx, "check.winv", sizeof tbl, (void**)&d_winv));
  BP_TRY(ws_get(ctx, "check.count", cells * sizeof(uint32_t), (void**)&d_count));
  uint32_t* target = nullptr;
  BP_HIP(ctx, hipMalloc((void**)&target, cells * sizeof(uint32_t)));
  unsigned long long h[4] = {0, 0, ~0ull, ~0ull};
  auto run = [&]() -> int {
    BP_HIP(ctx, hipMemcpyAsync(d_winv, &tbl, sizeof tbl, hipMemcpyHostToDevice, ctx->stream));
    BP_TRY(status_begin(ctx, &status));
    BP_HIP(ctx, hipEventRecord(ev0, ctx->stream));
    hipLaunchKernelGGL(sigma_decode, blocks_of(cells), dim3(256), 0, ctx->stream, e.lag + 5 * n, e.log_n, k, d_winv, target, status);
    BP_HIP(ctx, hipGetLastError());
    BP_HIP(ctx, hipMemsetAsync(d_count, 0, cells * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(sigma_indegree_count, blocks_of(cells), dim3(256), 0, ctx->stream, target, cells, d_count);
    BP_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(sigma_indegree_report, blocks_of(cells), dim3(256), 0, ctx->stream, d_count, cells, status);
    BP_HIP(ctx, hipGetLastError());
    BP_HIP(ctx, hipEventRecord(ev1, ctx->stream));
    BP_HIP(ctx, hipMemcpyAsync(h, status, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    BP_HIP(ctx, stream_wait(ctx->stream));
    BP_HIP(ctx, hipEventElapsedTime(decode_ms, ev0, ev1));
    return BP_OK;
  };
  const int rc = run();
  if (rc != BP_OK) {
    (void)hipFree(target);
    return rc;
  }
  e.sigma_target = target;
  const uint64_t rep[4] = {h[0], h[2], h[1], h[3]};
  memcpy(e.sigma_report, rep, sizeof rep);
  return BP_OK;
}

}  // namespace

int bp_circuit_check_sigma(bp_ctx* ctx, uint64_t circuit_handle, uint64_t report[4]) {
  if (!ctx || !report) return BP_ERR_INVALID_ARG;
  auto it = ctx->circuits.find(circuit_handle);
  if (it == ctx->circuits.end()) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "unknown circuit handle");
  DeviceGuard guard(ctx->device);
  hipEvent_t* ev;
  BP_TRY(check_events(ctx, &ev));
  float decode_ms = 0;
  BP_TRY(sigma_ensure(ctx, it->second, ev[0], ev[1], &decode_ms));
  const float ms[3] = {decode_ms, 0, 0};
  memcpy(ctx->check_ms, ms, sizeof ms);
  memcpy(report, it->second.sigma_report, 4 * sizeof(uint64_t));
  return BP_OK;
}

int bp_circuit_check_witness(bp_ctx* ctx, uint64_t circuit_handle, const void* a, const void* b, const void* c, const void* public_input,
                             int scalar_fmt, int witness_on_device, uint64_t report[5]) {
  if (!ctx || !a || !b || !c || !report || !fmt_ok(scalar_fmt)) return BP_ERR_INVALID_ARG;
  if (witness_on_device && scalar_fmt != BP_FR_MONT) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "device witness must be Montgomery");
  auto it = ctx->circuits.find(circuit_handle);
  if (it == ctx->circuits.end()) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "unknown circuit handle");
  CircuitEntry& cir = it->second;
  const size_t n = (size_t)1 << cir.log_n;
  DeviceGuard guard(ctx->device);
  hipEvent_t* ev;
  BP_TRY(check_events(ctx, &ev));
  float ms[3] = {0, 0, 0};
  BP_TRY(sigma_ensure(ctx, cir, ev[0], ev[1], &ms[0]));
  if (cir.sigma_report[0] || cir.sigma_report[2]) {
    const uint64_t cell = cir.sigma_report[0] ? cir.sigma_report[1] : cir.sigma_report[3];
    char msg[200];
    snprintf(msg, sizeof msg, "sigma is not a permutation, see bp_circuit_check_sigma: lowest bad cell %llu (row %llu of S%llu): %s",
             (unsigned long long)cell, (unsigned long long)(cell / 3), (unsigned long long)(cell % 3 + 1),
             cir.sigma_report[0] ? "its value is no cell label" : "it is not the target of exactly one cell");
    return BP_FAIL(ctx, BP_ERR_INVALID_ARG, msg);
  }
  // the witness where the kernel reads it: in place on the device, else uploaded to a workspace of this call's own
  const void* src[4] = {a, b, c, public_input};
  const fr_t* col[4] = {(const fr_t*)a, (const fr_t*)b, (const fr_t*)c, (const fr_t*)public_input};
  uint32_t* d_bad = nullptr;
  BP_HIP(ctx, hipEventRecord(ev[2], ctx->stream));
  if (!witness_on_device) {
    fr_t* wit;
    BP_TRY(ws_get(ctx, "check.witness", 4 * n * sizeof(fr_t), (void**)&wit));
    const size_t count = public_input ? 4 : 3;
    for (size_t k = 0; k < count; k++) {
      BP_HIP(ctx, hipMemcpyAsync(wit + k * n, src[k], n * sizeof(fr_t), hipMemcpyHostToDevice, ctx->stream));
      col[k] = wit + k * n;
    }
    BP_TRY(fr_bad_word(ctx, scalar_fmt, &d_bad));
    if (scalar_fmt == BP_FR_BYTES_LE) BP_TRY(fr_convert_run(ctx, wit, count * n, 0, d_bad));
  }
  BP_HIP(ctx, hipEventRecord(ev[3], ctx->stream));
  unsigned long long* status;
  BP_TRY(status_begin(ctx, &status));
  BP_HIP(ctx, hipEventRecord(ev[4], ctx->stream));
  hipLaunchKernelGGL(witness_check, blocks_of(n), dim3(256), 0, ctx->stream, col[0], col[1], col[2], col[3], cir.lag, n, cir.sigma_target, status);
  BP_HIP(ctx, hipGetLastError());
  BP_HIP(ctx, hipEventRecord(ev[5], ctx->stream));
  unsigned long long h[4] = {0, 0, ~0ull, ~0ull};
  uint32_t bad = 0;
  BP_HIP(ctx, hipMemcpyAsync(h, status, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  if (d_bad) BP_HIP(ctx, hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
  BP_HIP(ctx, stream_wait(ctx->stream));
  if (bad) return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, "witness element >= q");
  BP_HIP(ctx, hipEventElapsedTime(&ms[1], ev[2], ev[3]));
  BP_HIP(ctx, hipEventElapsedTime(&ms[2], ev[4], ev[5]));
  memcpy(ctx->check_ms, ms, sizeof ms);
  report[0] = h[0];
  report[1] = h[2];
  report[2] = h[1];
  report[3] = h[3] == ~0ull ? ~0ull : h[3] >> 32;
  report[4] = h[3] == ~0ull ? ~0ull : h[3] & 0xffffffffull;
  return BP_OK;
}

int bp_circuit_check_last_stats(bp_ctx* ctx, float stage_ms[3]) {
  if (!ctx || !stage_ms) return BP_ERR_INVALID_ARG;
  memcpy(stage_ms, ctx->check_ms, 3 * sizeof(float));
  return BP_OK;
}

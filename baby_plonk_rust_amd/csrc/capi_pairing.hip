// capi_pairing.hip -- C ABI, part 8: the pairing checks that turn the pairs of bp_verify_reduce(_segments) into verdicts
// (verifier.rs:187-191).  bp_g2_mul_generator, bp_pairing_gt_host and bp_pairing_check_host are host code over pairing_host.hpp;
// bp_pairing_check runs the same pairing.hpp one check per GPU lane (pairing_kernels.hpp).  All G2 work -- decoding x_2, its curve and
// subgroup tests, the prepared lines of x_2 and of the generator -- is host work done once per call.
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "ctx.hpp"
#include "pairing_host.hpp"
#include "pairing_kernels.hpp"

#include "capi_common.hpp"

using namespace bp;

int bp_g2_mul_generator(const uint8_t k32[32], uint8_t out192[192]) {
  if (!k32 || !out192) return BP_ERR_INVALID_ARG;
  return host_g2_mul_generator(k32, out192);
}

int bp_pairing_gt_host(const uint8_t p96[96], const uint8_t q192[192], uint8_t gt576[576]) {
  if (!p96 || !q192 || !gt576) return BP_ERR_INVALID_ARG;
  return host_pairing_gt(p96, q192, gt576);
}

int bp_pairing_check_host(const uint8_t x2_192[192], const uint8_t* pairs192, size_t n, uint32_t checks, uint8_t* verdicts,
                          uint8_t* gt576_or_null, size_t* first_bad) {
  return host_pairing_check(x2_192, pairs192, n, checks, verdicts, gt576_or_null, first_bad);
}

// lanes per pass: the workspace is PAIRING_SLOTS x 96 bytes per lane (5.8 KB), so a pass of 2^15 lanes holds 189 MB and fills the
// 256 CUs with two waves each; a longer call reuses the workspace pass after pass
constexpr size_t PAIRING_PASS_LANES = (size_t)1 << 15;

static int pairing_check_run(bp_ctx* ctx, const g2_affine& x2, const uint8_t* pairs192, size_t n, uint32_t checks, uint8_t* verdicts,
                             uint8_t* gt576_or_null, size_t* first_bad) {
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<fp2_t> lines(2 * PAIRING_TABLE_FP2);
  g2_prepare(lines.data(), x2);
  memcpy(lines.data() + PAIRING_TABLE_FP2, g2_generator_lines(), PAIRING_TABLE_FP2 * sizeof(fp2_t));

  const size_t pass = std::min(n, PAIRING_PASS_LANES), stride = (pass + 63) / 64 * 64;
  uint8_t *d_recs, *d_verdicts;
  g1_affine* d_pts;
  fp2_t* d_lines;
  unsigned long long* d_status;
  uint32_t *d_ws, *d_gt = nullptr;
  BP_TRY(ws_get(ctx, "pairing.records", n * 192, (void**)&d_recs));
  BP_TRY(ws_get(ctx, "pairing.points", 2 * n * sizeof(g1_affine), (void**)&d_pts));
  BP_TRY(ws_get(ctx, "pairing.lines", lines.size() * sizeof(fp2_t), (void**)&d_lines));
  BP_TRY(ws_get(ctx, "pairing.status", 8, (void**)&d_status));
  BP_TRY(ws_get(ctx, "pairing.ws", pairing_ws_dwords(stride) * sizeof(uint32_t), (void**)&d_ws));
  BP_TRY(ws_get(ctx, "pairing.verdicts", n, (void**)&d_verdicts));
  if (gt576_or_null) BP_TRY(ws_get(ctx, "pairing.gt", n * GT_BYTES, (void**)&d_gt));
  hipEvent_t* ev;                                                   // the four boundaries of the three stages
  BP_TRY(ev_get(ctx, "pairing", 4, hipEventDefault, &ev));
  hipStream_t st = ctx->stream;
  const float prepare_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();      // the lines: host work
  const StreamDrain drain{st};                                      // the copies below read the lines and the caller's pairs: pageable memory of this call
  auto blocks = [](size_t lanes) { return dim3((unsigned)((lanes + 63) / 64)); };

  // stage 0: upload, decode and check the 2 n points; the call waits here and reads the status word
  BP_HIP(ctx, hipEventRecord(ev[0], st));
  BP_HIP(ctx, hipMemcpyAsync(d_recs, pairs192, n * 192, hipMemcpyHostToDevice, st));
  BP_HIP(ctx, hipMemcpyAsync(d_lines, lines.data(), lines.size() * sizeof(fp2_t), hipMemcpyHostToDevice, st));
  BP_HIP(ctx, hipMemsetAsync(d_status, 0xff, 8, st));
  hipLaunchKernelGGL(pairing_decode, blocks(2 * n), dim3(64), 0, st, d_recs, 2 * n, checks & PAIRING_CHECK_G1_SUBGROUP, d_pts, d_status);
  BP_HIP(ctx, hipGetLastError());
  unsigned long long bad = ~0ull;
  BP_HIP(ctx, hipMemcpyAsync(&bad, d_status, 8, hipMemcpyDeviceToHost, st));
  BP_HIP(ctx, hipEventRecord(ev[1], st));
  BP_HIP(ctx, stream_wait(st));
  BP_HIP(ctx, hipEventElapsedTime(&ctx->pairing_ms[0], ev[0], ev[1]));
  ctx->pairing_ms[0] += prepare_ms;
  if (bad != ~0ull) {
    *first_bad = (size_t)(bad >> 2);
    char msg[160];
    snprintf(msg, sizeof msg, "pair %llu: a point rejected: %s", (unsigned long long)(bad >> 2), g1_reject_text((uint32_t)(bad & 3), false));
    return BP_FAIL(ctx, BP_ERR_BAD_POINT, msg);
  }

  // stages 1 and 2, pass by pass over the one workspace
  for (size_t first = 0; first < n; first += pass) {
    const size_t count = std::min(pass, n - first);
    BP_HIP(ctx, hipEventRecord(ev[1], st));
    hipLaunchKernelGGL(pairing_miller, blocks(count), dim3(64), 0, st, d_pts, first, count, d_lines, d_lines + PAIRING_TABLE_FP2, d_ws, stride);
    BP_HIP(ctx, hipGetLastError());
    BP_HIP(ctx, hipEventRecord(ev[2], st));
    hipLaunchKernelGGL(pairing_final, blocks(count), dim3(64), 0, st, first, count, d_ws, stride, d_verdicts, d_gt);
    BP_HIP(ctx, hipGetLastError());
    BP_HIP(ctx, hipEventRecord(ev[3], st));
    if (first + count == n) {
      BP_HIP(ctx, hipMemcpyAsync(verdicts, d_verdicts, n, hipMemcpyDeviceToHost, st));
      if (gt576_or_null) BP_HIP(ctx, hipMemcpyAsync(gt576_or_null, d_gt, n * GT_BYTES, hipMemcpyDeviceToHost, st));
    }
    BP_HIP(ctx, stream_wait(st));
    float ms[2];
    BP_HIP(ctx, hipEventElapsedTime(&ms[0], ev[1], ev[2]));
    BP_HIP(ctx, hipEventElapsedTime(&ms[1], ev[2], ev[3]));
    ctx->pairing_ms[1] += ms[0];
    ctx->pairing_ms[2] += ms[1];
  }
  return BP_OK;
}

int bp_pairing_check(bp_ctx* ctx, const uint8_t x2_192[192], const uint8_t* pairs192, size_t n, uint32_t checks, uint8_t* verdicts,
                     uint8_t* gt576_or_null, size_t* first_bad) {
  if (!ctx || !pairing_args_ok(x2_192, pairs192, n, verdicts, first_bad)) return BP_ERR_INVALID_ARG;
  *first_bad = SIZE_MAX;
  for (float& v : ctx->pairing_ms) v = 0;
  g2_affine x2;
  const int rc = pairing_decode_x2(x2, x2_192, checks);
  if (rc == BP_ERR_INVALID_ARG) return BP_FAIL(ctx, rc, "bp_pairing_check: x_2 is the identity (tau = 0 is not a setup)");
  if (rc != BP_OK) return BP_FAIL(ctx, rc, "bp_pairing_check: x_2 rejected (encoding, flags, not on the curve, or not in the subgroup)");
  if (n == 0) return BP_OK;
  if (n > ((size_t)1 << 30)) return BP_FAIL(ctx, BP_ERR_TOO_LARGE, "bp_pairing_check: more than 2^30 pairs");
  DeviceGuard guard(ctx->device);
  return pairing_check_run(ctx, x2, pairs192, n, checks, verdicts, gt576_or_null, first_bad);
}

int bp_pairing_last_stats(bp_ctx* ctx, float stage_ms[3]) {
  if (!ctx || !stage_ms) return BP_ERR_INVALID_ARG;
  for (int k = 0; k < 3; k++) stage_ms[k] = ctx->pairing_ms[k];
  return BP_OK;
}

// srs.hip -- host drivers of the SRS kernels (srs_kernels.hpp).
#include <stdlib.h>
#include <string.h>

#include <utility>
#include <vector>

#include "ctx.hpp"
#include "srs_kernels.hpp"

namespace bp {

int srs_decode_run(bp_ctx* ctx, const uint8_t* d_bytes, size_t n, g1_affine* d_out) {
  if (n == 0) return BP_OK;
  uint32_t* status;
  BP_TRY(ws_get(ctx, "srs.status", 4, (void**)&status));
  BP_HIP(ctx, hipMemsetAsync(status, 0, 4, ctx->stream));
  hipLaunchKernelGGL(srs_decode96, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_bytes, n, d_out, status);
  BP_HIP(ctx, hipGetLastError());
  uint32_t h = 0;
  BP_HIP(ctx, hipMemcpyAsync(&h, status, 4, hipMemcpyDeviceToHost, ctx->stream));
  BP_HIP(ctx, stream_wait(ctx->stream));
  if (h) return BP_FAIL(ctx, BP_ERR_BAD_POINT, h & 1 ? "non-canonical point encoding" : "point not on the curve");
  return BP_OK;
}
int srs_encode_run(bp_ctx* ctx, const g1_affine* d_in, size_t n, uint8_t* d_bytes) {
  if (n == 0) return BP_OK;
  hipLaunchKernelGGL(srs_encode96, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_in, n, d_bytes);
  BP_HIP(ctx, hipGetLastError());
  return BP_OK;
}
// compressed records -> points (+ the subgroup test when `subgroup`); *bad = ~0 when every point passed, else the status word of
// srs_kernels.hpp: (lowest failing index << 2) | reason, the index local to d_bytes
static int status_begin(bp_ctx* ctx, unsigned long long** status) {
  BP_TRY(ws_get(ctx, "srs.status64", 8, (void**)status));
  BP_HIP(ctx, hipMemsetAsync(*status, 0xff, 8, ctx->stream));
  return BP_OK;
}
static int status_read(bp_ctx* ctx, const unsigned long long* status, uint64_t* bad) {
  BP_HIP(ctx, hipGetLastError());
  unsigned long long h = ~0ull;
  BP_HIP(ctx, hipMemcpyAsync(&h, status, 8, hipMemcpyDeviceToHost, ctx->stream));
  BP_HIP(ctx, stream_wait(ctx->stream));
  *bad = h;
  return BP_OK;
}
int srs_decode48_run(bp_ctx* ctx, const uint8_t* d_bytes, size_t n, bool subgroup, g1_affine* d_out, uint64_t* bad) {
  *bad = ~0ull;
  if (n == 0) return BP_OK;
  unsigned long long* status;
  BP_TRY(status_begin(ctx, &status));
  const dim3 grid((unsigned)((n + 255) / 256));
  hipLaunchKernelGGL(srs_decode48, grid, dim3(256), 0, ctx->stream, d_bytes, n, d_out, status);
  if (subgroup) hipLaunchKernelGGL(srs_subgroup_check, grid, dim3(256), 0, ctx->stream, d_out, n, status);
  return status_read(ctx, status, bad);
}
int srs_subgroup_run(bp_ctx* ctx, const g1_affine* d_pts, size_t n, uint64_t* bad) {
  *bad = ~0ull;
  if (n == 0) return BP_OK;
  unsigned long long* status;
  BP_TRY(status_begin(ctx, &status));
  hipLaunchKernelGGL(srs_subgroup_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_pts, n, status);
  return status_read(ctx, status, bad);
}
int srs_encode48_run(bp_ctx* ctx, const g1_affine* d_in, size_t n, uint8_t* d_bytes) {
  if (n == 0) return BP_OK;
  hipLaunchKernelGGL(srs_encode48, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_in, n, d_bytes);
  BP_HIP(ctx, hipGetLastError());
  return BP_OK;
}
int srs_from_projective_run(bp_ctx* ctx, const g1_proj* d_in, size_t n, g1_affine* d_out) {
  if (n == 0) return BP_OK;
  // points per inversion: 2^16 lanes (one wave per SIMD), 8..64 points each.  Measured at 2^20 points (load of the literal seam):
  // 4.55 / 3.90 / 4.00 / 4.25 ms at 8 / 16 / 32 / 64 -- fewer inversions against a longer dependent chain through memory
  uint32_t group = 8;
  while (group < 64 && (n / group) > 65536) group <<= 1;
  {
    const char* v = knob("BP_SRS_PROJ_GROUP");        // experiment knob
    if (v) {
      const long g = strtol(v, nullptr, 10);
      if (g >= 1 && g <= 4096) group = (uint32_t)g;
    }
  }
  const size_t lanes = (n + group - 1) / group;
  hipLaunchKernelGGL(srs_from_projective, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, ctx->stream, d_in, n, group, d_out);
  BP_HIP(ctx, hipGetLastError());
  return BP_OK;
}
int srs_scale_run(bp_ctx* ctx, const g1_affine* d_pts, const fr_t* d_scalars, size_t n, g1_proj* d_out) {
  if (n == 0) return BP_OK;
  hipLaunchKernelGGL(srs_scale, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_pts, d_scalars, n, d_out);
  BP_HIP(ctx, hipGetLastError());
  return BP_OK;
}
int srs_generate_run(bp_ctx* ctx, const fr_t& a, const fr_t& d, int mode, size_t first, size_t n, g1_affine* d_out) {
  if (n == 0) return BP_OK;
  // the table of the generator's multiples (1 MiB) lives in a workspace of the context: built by the first call, in stream order
  // (ctx->gen_table_ready: set only after the table kernel was accepted by the runtime -- the workspace map gains its entry before
  // the allocation, so the map alone would call a table "there" after a failed first call)
  g1_affine28* table;
  BP_TRY(ws_get(ctx, "srs.gen_table", (size_t)GEN_WINDOWS * GEN_DIGITS * sizeof(g1_affine28), (void**)&table));
  if (!ctx->gen_table_ready || ctx->gen_table_ptr != (const void*)table) {
    hipLaunchKernelGGL(srs_gen_table, dim3((GEN_WINDOWS * GEN_DIGITS + 255) / 256), dim3(256), 0, ctx->stream, table);
    BP_HIP(ctx, hipGetLastError());
    ctx->gen_table_ready = true;
    ctx->gen_table_ptr = table;
  }
  const size_t lanes = (n + SRS_GEN_GROUP - 1) / SRS_GEN_GROUP;
  hipLaunchKernelGGL(srs_generate_fb, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, ctx->stream, a, d, mode, first, n, table, d_out);
  BP_HIP(ctx, hipGetLastError());
  return BP_OK;
}

// d_out[i] = (i_ntt_381 over G1 of d_in[0 .. 2^log_n))_i, affine: log_n passes of g1_ntt_pass over two projective buffers (pass 0
// reads d_in itself: lift, bit reversal and the n^-1 scaling are part of it), then the shared-inversion normalisation every
// projective SRS load goes through.  Enqueued on ctx->stream and waited for: the pass times (the context's "srs.g1_ntt" events, one
// more than the longest transform so far has passes) are read before it returns.
int g1_ntt_run(bp_ctx* ctx, const g1_affine* d_in, uint32_t log_n, g1_affine* d_out) {
  ctx->g1_ntt_pass_ms.clear();
  if (log_n > G1_NTT_MAX_LOG) return BP_FAIL(ctx, BP_ERR_TOO_LARGE, "G1 transform longer than 2^24");
  if (log_n == 0) {                                    // n = 1: L_0 = P_0
    BP_HIP(ctx, hipMemcpyAsync(d_out, d_in, sizeof(g1_affine), hipMemcpyDeviceToDevice, ctx->stream));
    BP_HIP(ctx, stream_wait(ctx->stream));
    return BP_OK;
  }
  const size_t n = (size_t)1 << log_n, half = n >> 1;
  g1_proj *src, *dst;
  fr_t* tw;
  BP_TRY(ws_get(ctx, "srs.g1_ntt_a", n * sizeof(g1_proj), (void**)&dst));
  BP_TRY(ws_get(ctx, "srs.g1_ntt_b", n * sizeof(g1_proj), (void**)&src));
  BP_TRY(ws_get(ctx, "srs.g1_ntt_tw", half * sizeof(fr_t), (void**)&tw));
  fr_t omega, n_inv = finv(fr_from_u64((uint64_t)n));
  (void)host_root_of_unity(omega, (uint64_t)n);
  Fr::from_mont(n_inv, n_inv);
  BP_TRY(roots_run(ctx, omega, half, tw));             // omega_n^k, k < n / 2
  hipEvent_t* ev;
  BP_TRY(ev_get(ctx, "srs.g1_ntt", log_n + 1, hipEventDefault, &ev));
  const dim3 grid((unsigned)((half + 255) / 256));
  BP_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
  for (uint32_t s = 0; s < log_n; s++) {
    if (s == 0) hipLaunchKernelGGL(g1_ntt_pass<true>, grid, dim3(256), 0, ctx->stream, log_n, s, d_in, (const g1_proj*)nullptr, dst, tw, n_inv);
    else hipLaunchKernelGGL(g1_ntt_pass<false>, grid, dim3(256), 0, ctx->stream, log_n, s, (const g1_affine*)nullptr, src, dst, tw, n_inv);
    BP_HIP(ctx, hipGetLastError());
    BP_HIP(ctx, hipEventRecord(ev[s + 1], ctx->stream));
    std::swap(src, dst);
  }
  BP_TRY(srs_from_projective_run(ctx, src, n, d_out));
  BP_HIP(ctx, stream_wait(ctx->stream));
  for (uint32_t s = 0; s < log_n; s++) {
    float ms = 0;
    BP_HIP(ctx, hipEventElapsedTime(&ms, ev[s], ev[s + 1]));
    ctx->g1_ntt_pass_ms.push_back(ms);
  }
  return BP_OK;
}

// ---- all n proofs of a polynomial on its domain (kzg_open_all.hpp) ------------------------------------------------------------------
// The two projective buffers (2n points each; the Lagrange transform's, grown) and the twiddles of both lengths: omega_2n^k, k < n, then omega_n^k, k < n / 2.
struct OpenAllBufs {
  g1_proj *a, *b;
  fr_t *tw_big, *tw_small;
};
static int open_all_bufs(bp_ctx* ctx, uint32_t log_n, OpenAllBufs* o) {
  const size_t n = (size_t)1 << log_n;
  fr_t* tw;
  BP_TRY(ws_get(ctx, "srs.g1_ntt_a", 2 * n * sizeof(g1_proj), (void**)&o->a));
  BP_TRY(ws_get(ctx, "srs.g1_ntt_b", 2 * n * sizeof(g1_proj), (void**)&o->b));
  BP_TRY(ws_get(ctx, "kzg.oa_tw", (n + n / 2 + 1) * sizeof(fr_t), (void**)&tw));
  o->tw_big = tw;
  o->tw_small = tw + n;
  if (ctx->open_all_tw_ptr == (const void*)tw && ctx->open_all_tw_log_n == log_n) return BP_OK;      // kept between calls of one size
  ctx->open_all_tw_ptr = nullptr;
  fr_t omega;
  (void)host_root_of_unity(omega, (uint64_t)(2 * n));
  BP_TRY(roots_run(ctx, omega, n, o->tw_big));
  (void)host_root_of_unity(omega, (uint64_t)n);
  BP_TRY(roots_run(ctx, omega, n / 2, o->tw_small));
  ctx->open_all_tw_ptr = tw;
  ctx->open_all_tw_log_n = log_n;
  return BP_OK;
}
int open_all_twiddles_run(bp_ctx* ctx, uint32_t log_n) {
  OpenAllBufs w;
  return open_all_bufs(ctx, log_n, &w);
}
// passes 1 .. log_len - 1 behind a pass 0 that wrote *cur (the other buffer: *oth); on return *cur holds the result.  ev[s + 1] is
// recorded behind pass s (ev[0]: the caller's, in front of pass 0).
static int open_all_rest_run(bp_ctx* ctx, uint32_t log_len, const fr_t* tw, g1_proj** cur, g1_proj** oth, hipEvent_t* ev) {
  const size_t half = (size_t)1 << (log_len - 1);
  const dim3 grid((unsigned)((half + 255) / 256));
  BP_HIP(ctx, hipGetLastError());                        // pass 0's launch
  BP_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
  for (uint32_t s = 1; s < log_len; s++) {
    hipLaunchKernelGGL(g1_ntt_pass<false>, grid, dim3(256), 0, ctx->stream, log_len, s, (const g1_affine*)nullptr, (const g1_proj*)*cur, *oth, tw, Fr::zero());
    BP_HIP(ctx, hipGetLastError());
    BP_HIP(ctx, hipEventRecord(ev[s + 1], ctx->stream));
    std::swap(*cur, *oth);
  }
  return BP_OK;
}
static int open_all_pass_times(bp_ctx* ctx, hipEvent_t* ev, uint32_t passes) {
  for (uint32_t s = 0; s < passes; s++) {
    float ms = 0;
    BP_HIP(ctx, hipEventElapsedTime(&ms, ev[s], ev[s + 1]));
    ctx->g1_ntt_pass_ms.push_back(ms);
  }
  return BP_OK;
}
// d_table[0 .. 2n) = DFT_2n(S^) of the first n - 1 points of d_srs, affine, natural order.  Waits for the stream; its log_n + 1 pass
// times are appended to ctx->g1_ntt_pass_ms.  1 <= log_n < G1_NTT_MAX_LOG.
int open_all_table_run(bp_ctx* ctx, const g1_affine* d_srs, uint32_t log_n, g1_affine* d_table) {
  const size_t n = (size_t)1 << log_n;
  OpenAllBufs w;
  BP_TRY(open_all_bufs(ctx, log_n, &w));
  hipEvent_t* ev;
  BP_TRY(ev_get(ctx, "kzg.oa_table", log_n + 2, hipEventDefault, &ev));
  g1_proj *cur = w.a, *oth = w.b;
  BP_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
  hipLaunchKernelGGL(g1_ntt_table_pass0, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, log_n, d_srs, cur);
  BP_TRY(open_all_rest_run(ctx, log_n + 1, w.tw_big, &cur, &oth, ev));
  BP_TRY(srs_from_projective_run(ctx, cur, 2 * n, d_table));
  BP_HIP(ctx, stream_wait(ctx->stream));
  return open_all_pass_times(ctx, ev, log_n + 1);
}
// d_out[i] = proof i, affine: the Toeplitz transform over d_table with the per-entry scalars d_sc = N^-1 DFT_2n(c^) (Montgomery), the
// final transform over its first n outputs, the normalisation.  `mid` is recorded between the two transforms.  Waits for the stream;
// appends the log_n + 1 and log_n pass times.
int open_all_proofs_run(bp_ctx* ctx, const g1_affine* d_table, const fr_t* d_sc, uint32_t log_n, g1_affine* d_out, hipEvent_t mid) {
  const size_t n = (size_t)1 << log_n;
  OpenAllBufs w;
  BP_TRY(open_all_bufs(ctx, log_n, &w));
  hipEvent_t* ev;
  BP_TRY(ev_get(ctx, "kzg.oa_proofs", 2 * log_n + 3, hipEventDefault, &ev));
  hipEvent_t* ev2 = ev + log_n + 2;
  g1_proj *cur = w.a, *oth = w.b;
  BP_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
  const dim3 grid0((unsigned)((n + 255) / 256));
#ifdef BP_EXPERIMENT
  const char* mul = knob("BP_OPEN_ALL_MUL");              // experiment knob: split28 = the 128-step multiplication of srs_scale in pass 0
  if (mul && !strcmp(mul, "split28")) hipLaunchKernelGGL(g1_ntt_toeplitz_pass0_split28, grid0, dim3(256), 0, ctx->stream, log_n + 1, d_table, d_sc, cur);
  else
#endif
    hipLaunchKernelGGL(g1_ntt_toeplitz_pass0, grid0, dim3(256), 0, ctx->stream, log_n + 1, d_table, d_sc, cur);
  BP_TRY(open_all_rest_run(ctx, log_n + 1, w.tw_big, &cur, &oth, ev));
  BP_HIP(ctx, hipEventRecord(mid, ctx->stream));
  BP_HIP(ctx, hipEventRecord(ev2[0], ctx->stream));
  hipLaunchKernelGGL(g1_ntt_final_pass0, dim3((unsigned)((n / 2 + 255) / 256)), dim3(256), 0, ctx->stream, log_n, (const g1_proj*)cur, oth);
  std::swap(cur, oth);                                   // cur: what pass 0 wrote; oth: h, free from pass 1 on
  BP_TRY(open_all_rest_run(ctx, log_n, w.tw_small, &cur, &oth, ev2));
  BP_TRY(srs_from_projective_run(ctx, cur, n, d_out));
  BP_HIP(ctx, stream_wait(ctx->stream));
  BP_TRY(open_all_pass_times(ctx, ev, log_n + 1));
  return open_all_pass_times(ctx, ev2, log_n);
}
// d_out[t] = scale c^_t, t < 2n (srs_kernels.hpp: open_all_chat_fill)
int open_all_chat_run(bp_ctx* ctx, uint32_t log_n, const fr_t* d_f, size_t n_values, const fr_t& scale, fr_t* d_out) {
  const size_t N = (size_t)2 << log_n;
  hipLaunchKernelGGL(open_all_chat_fill, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, log_n, d_f, n_values, scale, d_out);
  BP_HIP(ctx, hipGetLastError());
  return BP_OK;
}

// ---- the n / l cell proofs of a polynomial (kzg_open_cosets.hpp); log_l = 0 is open_all itself ---------------------------------------
// the two projective buffers at `points` points each, and the twiddles of the lengths R = 2r and r (open_all's, for log_r)
static int open_cosets_bufs(bp_ctx* ctx, uint32_t log_r, size_t points, OpenAllBufs* o) {
  BP_TRY(ws_get(ctx, "srs.g1_ntt_a", points * sizeof(g1_proj), (void**)&o->a));
  BP_TRY(ws_get(ctx, "srs.g1_ntt_b", points * sizeof(g1_proj), (void**)&o->b));
  return open_all_bufs(ctx, log_r, o);                   // grow-only workspaces: the same two buffers, not smaller
}
int open_cosets_twiddles_run(bp_ctx* ctx, uint32_t log_n, uint32_t log_l) {
  OpenAllBufs w;
  return open_cosets_bufs(ctx, log_n - log_l, (size_t)1 << log_n, &w);      // what open_cosets_proofs_run asks for
}
// ev[k] -> ev[k + 1]: launch k of a sequence
static inline int pass_mark(bp_ctx* ctx, hipEvent_t* ev, uint32_t* k) {
  BP_HIP(ctx, hipGetLastError());
  BP_HIP(ctx, hipEventRecord(ev[++*k], ctx->stream));
  return BP_OK;
}
// d_table[j R + i] = DFT_R(S^(j))_i, j < l, i < R = 2n / l, of the first n - l points of d_srs: affine.  Waits for the stream; appends
// its log_R pass times.  log_l < log_n < G1_NTT_MAX_LOG.
int open_cosets_table_run(bp_ctx* ctx, const g1_affine* d_srs, uint32_t log_n, uint32_t log_l, g1_affine* d_table) {
  if (log_l == 0) return open_all_table_run(ctx, d_srs, log_n, d_table);
  const size_t n = (size_t)1 << log_n;
  const uint32_t log_R = log_n - log_l + 1;
  OpenAllBufs w;
  BP_TRY(open_cosets_bufs(ctx, log_n - log_l, 2 * n, &w));
  hipEvent_t* ev;
  BP_TRY(ev_get(ctx, "kzg.oc_table", log_R + 1, hipEventDefault, &ev));
  g1_proj *cur = w.a, *oth = w.b;
  const dim3 grid((unsigned)((n + 255) / 256));          // l transforms of R / 2 butterflies: n lanes in every pass
  uint32_t k = 0;
  BP_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
  hipLaunchKernelGGL(g1_ntt_cosets_table_pass0, grid, dim3(256), 0, ctx->stream, log_n, log_l, d_srs, cur);
  BP_TRY(pass_mark(ctx, ev, &k));
  for (uint32_t s = 1; s < log_R; s++) {
    hipLaunchKernelGGL(g1_ntt_batch_pass, grid, dim3(256), 0, ctx->stream, log_R, log_l, s, (const g1_proj*)cur, oth, (const fr_t*)w.tw_big);
    BP_TRY(pass_mark(ctx, ev, &k));
    std::swap(cur, oth);
  }
  BP_TRY(srs_from_projective_run(ctx, cur, 2 * n, d_table));
  BP_HIP(ctx, stream_wait(ctx->stream));
  return open_all_pass_times(ctx, ev, log_R);
}
// d_out[k] = the proof of cell k < r, affine, from the table and d_sc[j R + i] = R^-1 DFT_R(c^(j))_i (Montgomery): the multiplication,
// the log_l - 1 halving passes, the inverse transform of length R, the final transform of length r, the normalisation.  `mid` is
// recorded in front of the final transform.  Waits for the stream; appends the log_l + log_R + log_r pass times in that order.
int open_cosets_proofs_run(bp_ctx* ctx, const g1_affine* d_table, const fr_t* d_sc, uint32_t log_n, uint32_t log_l, g1_affine* d_out, hipEvent_t mid) {
  if (log_l == 0) return open_all_proofs_run(ctx, d_table, d_sc, log_n, d_out, mid);
  const size_t n = (size_t)1 << log_n;
  const uint32_t log_r = log_n - log_l, log_R = log_r + 1, passes = log_l + log_R + log_r;
  const size_t r = (size_t)1 << log_r;
  OpenAllBufs w;
  BP_TRY(open_cosets_bufs(ctx, log_r, n, &w));           // n >= R: row 0 of the products, then both buffers of the transforms
  hipEvent_t* ev;
  BP_TRY(ev_get(ctx, "kzg.oc_proofs", passes + 1, hipEventDefault, &ev));
  g1_proj *cur = w.a, *oth = w.b;
  uint32_t k = 0;
  BP_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
  hipLaunchKernelGGL(g1_ntt_cosets_mul_pass, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, log_n, log_l, d_table, d_sc, cur);
  BP_TRY(pass_mark(ctx, ev, &k));
  for (size_t half = n >> 1; half >= 2 * r; half >>= 1) {
    hipLaunchKernelGGL(g1_ntt_cosets_halve_pass, dim3((unsigned)((half + 255) / 256)), dim3(256), 0, ctx->stream, (uint64_t)half, cur);
    BP_TRY(pass_mark(ctx, ev, &k));
  }
  for (uint32_t s = 0; s < log_R; s++) {
    hipLaunchKernelGGL(g1_ntt_pass<false>, dim3((unsigned)((r + 255) / 256)), dim3(256), 0, ctx->stream, log_R, s, (const g1_affine*)nullptr,
                       (const g1_proj*)cur, oth, (const fr_t*)w.tw_big, Fr::zero());
    BP_TRY(pass_mark(ctx, ev, &k));
    std::swap(cur, oth);
  }
  BP_HIP(ctx, hipEventRecord(mid, ctx->stream));
  hipLaunchKernelGGL(g1_ntt_final_pass0, dim3((unsigned)((r / 2 + 255) / 256)), dim3(256), 0, ctx->stream, log_r, (const g1_proj*)cur, oth);
  BP_TRY(pass_mark(ctx, ev, &k));
  std::swap(cur, oth);                                   // cur: what pass 0 wrote; oth: h, free from pass 1 on
  for (uint32_t s = 1; s < log_r; s++) {
    hipLaunchKernelGGL(g1_ntt_pass<false>, dim3((unsigned)((r / 2 + 255) / 256)), dim3(256), 0, ctx->stream, log_r, s, (const g1_affine*)nullptr,
                       (const g1_proj*)cur, oth, (const fr_t*)w.tw_small, Fr::zero());
    BP_TRY(pass_mark(ctx, ev, &k));
    std::swap(cur, oth);
  }
  BP_TRY(srs_from_projective_run(ctx, cur, r, d_out));
  BP_HIP(ctx, stream_wait(ctx->stream));
  return open_all_pass_times(ctx, ev, passes);
}
// d_out[j R + t] = scale c^(j)_t, j < l, t < R (srs_kernels.hpp: open_cosets_chat_fill)
int open_cosets_chat_run(bp_ctx* ctx, uint32_t log_n, uint32_t log_l, const fr_t* d_f, size_t n_values, const fr_t& scale, fr_t* d_out) {
  const size_t N = (size_t)2 << log_n;
  hipLaunchKernelGGL(open_cosets_chat_fill, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, log_n, log_l, d_f, n_values, scale, d_out);
  BP_HIP(ctx, hipGetLastError());
  return BP_OK;
}
// d_out[k l + j] = d_in[k + r j]: the n values in cell order; d_out must not be d_in
int open_cosets_cell_order_run(bp_ctx* ctx, uint32_t log_n, uint32_t log_l, const fr_t* d_in, fr_t* d_out) {
  const size_t n = (size_t)1 << log_n;
  hipLaunchKernelGGL(open_cosets_cell_order, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, log_n, log_l, d_in, d_out);
  BP_HIP(ctx, hipGetLastError());
  return BP_OK;
}

}  // namespace bp

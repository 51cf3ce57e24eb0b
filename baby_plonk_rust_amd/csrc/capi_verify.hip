// capi_verify.hip -- C ABI, part 7: batch verification.  bp_verify_reduce turns m proofs of one circuit into the two G1 points whose
// pairings decide the batch (Verifier::verify, src/verifier.rs:80-192, without its last line); bp_plonk_challenges is the verifier's
// transcript (compute_challengs, verifier.rs:193-209) on the host.  Kernels: verify_kernels.hpp; decoding and the subgroup test are
// the SRS loader's (srs.hip), both multiplications the table-free MSM over workspace points (msm.hip).
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx.hpp"
#include "g1_check.hpp"
#include "verify_kernels.hpp"
#include "verify_segments_kernels.hpp"

#include "capi_common.hpp"

using namespace bp;

static const char* const VERIFY_POINT_NAME[VERIFY_POINTS] = {"a_1", "b_1", "c_1", "z_1", "t_lo_1", "t_mid_1", "t_hi_1", "w_zeta_1", "w_zeta_omega_1"};
static const char* const VERIFY_EVAL_NAME[VERIFY_EVALS] = {"a_bar", "b_bar", "c_bar", "s1_bar", "s2_bar", "z_omega_bar"};

int bp_plonk_challenges(const uint8_t* proofs624, size_t m, int scalar_fmt, void* out, size_t* first_bad) {
  if (!fmt_ok(scalar_fmt) || (m && (!proofs624 || !out))) return BP_ERR_INVALID_ARG;
  if (first_bad) *first_bad = SIZE_MAX;
  for (size_t j = 0; j < m; j++) {
    const uint8_t* rec = proofs624 + (size_t)VERIFY_RECORD_BYTES * j;
    for (int k = 0; k < VERIFY_EVALS; k++)
      if (!fr_is_canonical(rec + 432 + 32 * k)) {
        if (first_bad) *first_bad = j;
        return BP_ERR_BAD_SCALAR;
      }
    uint32_t words[VERIFY_RECORD_WORDS];
    memcpy(words, rec, VERIFY_RECORD_BYTES);
    fr_t c[6];
    plonk_challenges(words, c, nullptr);
    for (int k = 0; k < 6; k++) {
      fr_t v = c[k];                                           // canonical limbs: the BP_FR_BYTES_LE image as it is
      if (scalar_fmt == BP_FR_MONT) Fr::to_mont(v, v);
      memcpy((uint8_t*)out + ((size_t)6 * j + k) * 32, &v, 32);
    }
  }
  return BP_OK;
}

// what stages 0-3 leave on the device for stage 4, whichever it is
struct VerifyStaged {
  hipEvent_t* ev = nullptr;                // the context's six "verify" events: the boundaries of the five stages, [0..4] recorded
  size_t m = 0, n_pts = 0, n_all = 0;      // proofs, 9 m proof points, 9 m + 9 points with the shared bases behind them
  fr_t *d_b = nullptr, *d_a = nullptr;     // verify_scalars' scal_b (9 m, and nine free slots behind) and scal_a (2 m)
  fr_t* d_sh = nullptr;                    // its per-proof shares of the nine shared-base scalars (9 m)
  g1_affine* d_pts = nullptr;              // the decoded points, column-major, then the nine shared bases
  g1_affine shared_pts[VERIFY_SHARED];     // the shared bases as uploaded: eight vk commitments and G
};

// Stages 0-3 of both entry points: upload, transcript, scalars (with the batch-wide shared sums behind scal_b), decode + subgroup
// check, and the rejection path that names the lowest proof.  Records ev[0..4]; returns with the stream idle.
static int verify_stages_0_3(bp_ctx* ctx, uint32_t log_n, const uint8_t vk768[768], const uint8_t* proofs624, size_t m, const void* public_inputs,
                             size_t n_public, const void* weights, const void* challenges, int fmt, size_t* first_bad, VerifyStaged* staged) {
  // the nine shared bases: eight vk commitments in the order bp_circuit_commitments writes them, then G
  g1_affine* shared_pts = staged->shared_pts;
  for (int k = 0; k < 8; k++)
    if (!host_point96(shared_pts[k], vk768 + 96 * k)) {
      char msg[96];
      snprintf(msg, sizeof msg, "verifier key: commitment %d rejected (encoding, flags or not on the curve)", k);
      return BP_FAIL(ctx, BP_ERR_BAD_POINT, msg);
    }
  shared_pts[8] = g1_affine_generator();
  VerifyParams P;
  if (!host_root_of_unity(P.omega, (uint64_t)1 << log_n)) return BP_ERR_INVALID_ARG;
  fr_invert(P.n_inv, fr_from_u64((uint64_t)1 << log_n));
  P.log_n = log_n;
  P.fmt = fmt;
  P.chal_fmt = challenges ? fmt : BP_FR_MONT;
  P.n_public = n_public;

  const size_t n_pts = (size_t)VERIFY_POINTS * m, n_all = n_pts + VERIFY_SHARED;
  uint8_t *d_rec, *d_comp;
  fr_t *d_chal, *d_w = nullptr, *d_pub = nullptr, *d_b, *d_a, *d_sh;
  g1_affine* d_pts;
  unsigned long long* d_status;
  BP_TRY(ws_get(ctx, "verify.records", m * VERIFY_RECORD_BYTES, (void**)&d_rec));
  BP_TRY(ws_get(ctx, "verify.comp", n_pts * 48, (void**)&d_comp));
  BP_TRY(ws_get(ctx, "verify.chal", m * 6 * sizeof(fr_t), (void**)&d_chal));
  if (weights) BP_TRY(ws_get(ctx, "verify.weights", m * sizeof(fr_t), (void**)&d_w));
  BP_TRY(ws_get(ctx, "verify.public", m * n_public * sizeof(fr_t), (void**)&d_pub));
  BP_TRY(ws_get(ctx, "verify.scal_b", n_all * sizeof(fr_t), (void**)&d_b));
  BP_TRY(ws_get(ctx, "verify.scal_a", 2 * m * sizeof(fr_t), (void**)&d_a));
  BP_TRY(ws_get(ctx, "verify.shared", n_pts * sizeof(fr_t), (void**)&d_sh));
  BP_TRY(ws_get(ctx, "verify.points", n_all * sizeof(g1_affine), (void**)&d_pts));
  BP_TRY(ws_get(ctx, "verify.status", 8, (void**)&d_status));
  hipEvent_t* ev;
  BP_TRY(ev_get(ctx, "verify", 6, hipEventDefault, &ev));
  hipStream_t st = ctx->stream;

  // stage 0: upload (pageable host memory: the copies are staged by the runtime before they return)
  BP_HIP(ctx, hipEventRecord(ev[0], st));
  BP_HIP(ctx, hipMemcpyAsync(d_rec, proofs624, m * VERIFY_RECORD_BYTES, hipMemcpyHostToDevice, st));
  if (challenges) BP_HIP(ctx, hipMemcpyAsync(d_chal, challenges, m * 6 * sizeof(fr_t), hipMemcpyHostToDevice, st));
  if (weights) BP_HIP(ctx, hipMemcpyAsync(d_w, weights, m * sizeof(fr_t), hipMemcpyHostToDevice, st));
  if (n_public) BP_HIP(ctx, hipMemcpyAsync(d_pub, public_inputs, m * n_public * sizeof(fr_t), hipMemcpyHostToDevice, st));
  BP_HIP(ctx, hipMemcpyAsync(d_pts + n_pts, shared_pts, sizeof staged->shared_pts, hipMemcpyHostToDevice, st));
  BP_HIP(ctx, hipMemsetAsync(d_status, 0xff, 8, st));
  // stage 1: transcript
  BP_HIP(ctx, hipEventRecord(ev[1], st));
  if (!challenges) {
    hipLaunchKernelGGL(verify_transcript, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st, d_rec, m, d_chal);
    BP_HIP(ctx, hipGetLastError());
  }
  // stage 2: scalars
  BP_HIP(ctx, hipEventRecord(ev[2], st));
  hipLaunchKernelGGL(verify_scalars, dim3((unsigned)((m + 127) / 128)), dim3(128), 0, st, d_rec, m, d_chal, d_w, d_pub, P, d_b, d_a, d_sh, d_status);
  BP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(verify_shared_sum, dim3(VERIFY_SHARED), dim3(256), 0, st, d_sh, m, d_b + n_pts);
  BP_HIP(ctx, hipGetLastError());
  unsigned long long scalar_bad = ~0ull;
  BP_HIP(ctx, hipMemcpyAsync(&scalar_bad, d_status, 8, hipMemcpyDeviceToHost, st));
  // stage 3: decode + subgroup check (the call waits for the stream and reads the status word)
  BP_HIP(ctx, hipEventRecord(ev[3], st));
  hipLaunchKernelGGL(verify_gather, dim3((unsigned)((n_pts + 255) / 256)), dim3(256), 0, st, d_rec, m, d_comp);
  BP_HIP(ctx, hipGetLastError());
  uint64_t point_bad = ~0ull;
  BP_TRY(srs_decode48_run(ctx, d_comp, n_pts, true, d_pts, &point_bad));
  BP_HIP(ctx, hipEventRecord(ev[4], st));

  if (point_bad != ~0ull || scalar_bad != ~0ull) {
    // The status word of the decoder is the lowest COLUMN-MAJOR index; the lowest proof may sit in a later column.  A rejection is
    // the rare path: ask column by column (nine short runs over data already decoded once) and keep the lowest proof.
    size_t pt_proof = SIZE_MAX;
    uint32_t pt_field = 0, pt_reason = 0;
    if (point_bad != ~0ull)
      for (int k = 0; k < VERIFY_POINTS; k++) {
        uint64_t bad = ~0ull;
        BP_TRY(srs_decode48_run(ctx, d_comp + (size_t)k * m * 48, m, true, d_pts + (size_t)k * m, &bad));
        if (bad != ~0ull && (size_t)(bad >> 2) < pt_proof) {
          pt_proof = (size_t)(bad >> 2);
          pt_field = (uint32_t)k;
          pt_reason = (uint32_t)(bad & 3);
        }
      }
    const size_t sc_proof = scalar_bad == ~0ull ? SIZE_MAX : (size_t)(scalar_bad >> 4);
    char msg[200];
    if (pt_proof != SIZE_MAX && pt_proof <= sc_proof) {            // on a tie the point is reported
      if (first_bad) *first_bad = pt_proof;
      snprintf(msg, sizeof msg, "proof %llu: point %s rejected: %s", (unsigned long long)pt_proof, VERIFY_POINT_NAME[pt_field],
               g1_reject_text(pt_reason, true));
      return BP_FAIL(ctx, BP_ERR_BAD_POINT, msg);
    }
    const uint32_t field = (uint32_t)(scalar_bad & 15);
    if (first_bad) *first_bad = sc_proof;
    snprintf(msg, sizeof msg, "proof %llu: %s is not a canonical scalar (>= q)", (unsigned long long)sc_proof,
             field < VERIFY_EVALS ? VERIFY_EVAL_NAME[field] : field == VERIFY_BAD_PUBLIC ? "a public input" : field == VERIFY_BAD_WEIGHT ? "the weight" : "a challenge");
    return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, msg);
  }

  staged->ev = ev;
  staged->m = m;
  staged->n_pts = n_pts;
  staged->n_all = n_all;
  staged->d_b = d_b;
  staged->d_a = d_a;
  staged->d_sh = d_sh;
  staged->d_pts = d_pts;
  return BP_OK;
}

static int verify_reduce_run(bp_ctx* ctx, uint32_t log_n, const uint8_t vk768[768], const uint8_t* proofs624, size_t m, const void* public_inputs,
                             size_t n_public, const void* weights, const void* challenges, int fmt, uint8_t out192[192], size_t* first_bad) {
  VerifyStaged V;
  BP_TRY(verify_stages_0_3(ctx, log_n, vk768, proofs624, m, public_inputs, n_public, weights, challenges, fmt, first_bad, &V));
  const size_t n_all = V.n_all;
  fr_t *d_b = V.d_b, *d_a = V.d_a;
  g1_affine* d_pts = V.d_pts;
  g1_affine28* d_p28;
  BP_TRY(ws_get(ctx, "verify.p28", n_all * sizeof(g1_affine28), (void**)&d_p28));
  hipStream_t st = ctx->stream;
  hipEvent_t* ev = V.ev;

  // stage 4: B over all 9 m + 9 points, A over the slice [7 m, 9 m) of the same array
  BP_TRY(srs_to28_into(ctx, d_pts, n_all, d_p28));
  MsmFlight f[2];                                                  // [0] B, [1] A
  int rc = msm_flight_launched(f[0], ctx, msm_launch(ctx, d_p28, n_all, d_b, BP_FR_MONT, 0, 0, 0, nullptr, &f[0].pend));
  if (rc == BP_OK) rc = msm_flight_launched(f[1], ctx, msm_launch(ctx, d_p28 + 7 * m, 2 * m, d_a, BP_FR_MONT, 0, 0, 1, nullptr, &f[1].pend));
  if (rc == BP_OK) {
    hipError_t he = hipEventRecord(ev[5], st);
    if (he != hipSuccess) rc = fail(ctx, BP_ERR_HIP, "hipEventRecord", he, __FILE__, __LINE__);
  }
  BP_TRY(msm_finish_all(ctx, f, 2, rc));
  for (int k = 0; k < 5; k++) BP_HIP(ctx, hipEventElapsedTime(&ctx->verify_ms[k], ev[k], ev[k + 1]));
  host_encode96(out192, f[1].out[0]);
  host_encode96(out192 + 96, f[0].out[0]);
  return BP_OK;
}

// the eight commitments of the verifier key all in the prime-order subgroup?  (The key is checked for the curve only: the reference
// verifier does no more.)  ~9 000 field products on the host, so the answer is kept with the key's bytes: a service verifies batch
// after batch against one key.
static bool vk_in_subgroup(bp_ctx* ctx, const uint8_t vk768[768], const g1_affine shared_pts[VERIFY_SHARED]) {
  if (ctx->verify_vk_seen.size() == 769 && memcmp(ctx->verify_vk_seen.data(), vk768, 768) == 0) return ctx->verify_vk_seen[768] != 0;
  bool ok = true;
  for (int k = 0; k < 8 && ok; k++) ok = g1_is_torsion_free(shared_pts[k]);
  ctx->verify_vk_seen.assign(vk768, vk768 + 768);
  ctx->verify_vk_seen.push_back(ok ? 1 : 0);
  return ok;
}

// Stage 4 of bp_verify_reduce_segments: T = 11 m + 9 S products, one per lane, then the sums (verify_segments_kernels.hpp).
static int verify_segments_run(bp_ctx* ctx, uint32_t log_n, const uint8_t vk768[768], const uint8_t* proofs624, size_t m, const void* public_inputs,
                               size_t n_public, const void* weights, const void* challenges, int fmt, size_t segment, uint8_t* out192,
                               size_t* first_bad) {
  VerifyStaged V;
  BP_TRY(verify_stages_0_3(ctx, log_n, vk768, proofs624, m, public_inputs, n_public, weights, challenges, fmt, first_bad, &V));
  const size_t seg = std::min(segment, m), S = (m + seg - 1) / seg;
  const size_t n_terms = (size_t)(VERIFY_POINTS + 2) * m, T = n_terms + (size_t)VERIFY_SHARED * S;
  fr_t* d_seg;
  uint32_t *d_prod, *d_node, *d_run;
  uint8_t* d_out;
  BP_TRY(ws_get(ctx, "verify.seg_scal", (size_t)VERIFY_SHARED * S * sizeof(fr_t), (void**)&d_seg));
  BP_TRY(ws_get(ctx, "verify.seg_prod", T * SEG_PT_WORDS * sizeof(uint32_t), (void**)&d_prod));
  BP_TRY(ws_get(ctx, "verify.seg_node", 2 * m * SEG_PT_WORDS * sizeof(uint32_t), (void**)&d_node));
  BP_TRY(ws_get(ctx, "verify.seg_run", 2 * S * N28 * sizeof(uint32_t), (void**)&d_run));
  BP_TRY(ws_get(ctx, "verify.seg_out", S * 192, (void**)&d_out));
  hipEvent_t *ev = V.ev, *sev;                                       // sev: the two boundaries inside stage 4
  BP_TRY(ev_get(ctx, "verify.seg", 2, hipEventDefault, &sev));
  hipStream_t st = ctx->stream;
  auto blocks = [](size_t n, size_t per) { return dim3((unsigned)((n + per - 1) / per)); };

  // the shared-base terms take the split form only where the endomorphism is [x^2]: on a key inside the subgroup
  size_t plain_from = vk_in_subgroup(ctx, vk768, V.shared_pts) ? T : n_terms;
  if (const char* v = knob("BP_VERIFY_SEG_PLAIN"))                  // experiment build: the A/B of docs/EXPERIMENTS.md
    if (*v && *v != '0') plain_from = 0;
  uint32_t L = 1;                                                   // lanes per segmented scalar sum
  while (L < 256 && L < seg) L <<= 1;
  hipLaunchKernelGGL(verify_seg_shared_sum, blocks((size_t)VERIFY_SHARED * S, 256 / L), dim3(256), 0, st, V.d_sh, m, seg, S, L, d_seg);
  BP_HIP(ctx, hipGetLastError());
  if (plain_from > 0) {
    hipLaunchKernelGGL(verify_seg_mul<true>, blocks(plain_from, 64), dim3(64), 0, st, V.d_pts, V.d_b, V.d_a, d_seg, m, S, (size_t)0, plain_from, d_prod);
    BP_HIP(ctx, hipGetLastError());
  }
  if (plain_from < T) {
    hipLaunchKernelGGL(verify_seg_mul<false>, blocks(T - plain_from, 64), dim3(64), 0, st, V.d_pts, V.d_b, V.d_a, d_seg, m, S, plain_from, T, d_prod);
    BP_HIP(ctx, hipGetLastError());
  }
  BP_HIP(ctx, hipEventRecord(sev[0], st));
  hipLaunchKernelGGL(verify_seg_proof_sum, blocks(2 * m, 64), dim3(64), 0, st, d_prod, T, m, d_node);
  BP_HIP(ctx, hipGetLastError());
  for (size_t d = 1; d < seg; d <<= 1) {
    const size_t slots = (seg + 2 * d - 1) / (2 * d);
    hipLaunchKernelGGL(verify_seg_tree, blocks(2 * S * slots, 64), dim3(64), 0, st, d_node, m, seg, S, d, slots);
    BP_HIP(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(verify_seg_add_shared, blocks(S, 64), dim3(64), 0, st, d_node, m, seg, S, d_prod, T);
  BP_HIP(ctx, hipGetLastError());
  BP_HIP(ctx, hipEventRecord(sev[1], st));
  // one inversion per pair at the least, per eight points where there are lanes to spare
  const uint32_t group = 2 * S >= ((size_t)1 << 15) ? 8 : 2 * S >= ((size_t)1 << 12) ? 4 : 2;
  hipLaunchKernelGGL(verify_seg_encode, blocks((2 * S + group - 1) / group, 64), dim3(64), 0, st, d_node, m, seg, S, group, d_run, d_out);
  BP_HIP(ctx, hipGetLastError());
  BP_HIP(ctx, hipEventRecord(ev[5], st));
  BP_HIP(ctx, hipMemcpyAsync(out192, d_out, S * 192, hipMemcpyDeviceToHost, st));
  BP_HIP(ctx, stream_wait(st));
  for (int k = 0; k < 5; k++) BP_HIP(ctx, hipEventElapsedTime(&ctx->verify_ms[k], ev[k], ev[k + 1]));
  BP_HIP(ctx, hipEventElapsedTime(&ctx->verify_seg_ms[0], ev[4], sev[0]));
  BP_HIP(ctx, hipEventElapsedTime(&ctx->verify_seg_ms[1], sev[0], sev[1]));
  BP_HIP(ctx, hipEventElapsedTime(&ctx->verify_seg_ms[2], sev[1], ev[5]));
  return BP_OK;
}

int bp_verify_reduce(bp_ctx* ctx, uint32_t log_n, const uint8_t vk768[768], const uint8_t* proofs624, size_t m, const void* public_inputs,
                     size_t n_public, const void* weights, const void* challenges, int scalar_fmt, uint8_t out192[192], size_t* first_bad) {
  if (!ctx || !vk768 || !out192 || !fmt_ok(scalar_fmt) || (m && !proofs624) || (m && n_public && !public_inputs)) return BP_ERR_INVALID_ARG;
  if (log_n < 3 || log_n > 28) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "bp_verify_reduce: log_n outside 3..28");
  if (!weights && m > 1) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "bp_verify_reduce: weights may be NULL for a single proof only");
  if (n_public > ((size_t)1 << log_n)) return BP_FAIL(ctx, BP_ERR_LENGTH, "bp_verify_reduce: more public inputs than rows");
  if (m >= (((size_t)1 << 31) - VERIFY_SHARED + VERIFY_POINTS - 1) / VERIFY_POINTS) return BP_FAIL(ctx, BP_ERR_TOO_LARGE, "bp_verify_reduce: 9 m + 9 >= 2^31 points");
  if (first_bad) *first_bad = SIZE_MAX;
  if (m == 0) {
    encode_identity_pair(out192);
    for (float& v : ctx->verify_ms) v = 0;
    return BP_OK;
  }
  DeviceGuard guard(ctx->device);
  for (float& v : ctx->verify_ms) v = 0;
  return verify_reduce_run(ctx, log_n, vk768, proofs624, m, public_inputs, n_public, weights, challenges, scalar_fmt, out192, first_bad);
}

int bp_verify_reduce_segments(bp_ctx* ctx, uint32_t log_n, const uint8_t vk768[768], const uint8_t* proofs624, size_t m, const void* public_inputs,
                              size_t n_public, const void* weights, const void* challenges, int scalar_fmt, size_t segment, uint8_t* out192,
                              size_t* first_bad) {
  if (!ctx || !vk768 || !fmt_ok(scalar_fmt) || (m && (!proofs624 || !out192)) || (m && n_public && !public_inputs)) return BP_ERR_INVALID_ARG;
  if (log_n < 3 || log_n > 28) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "bp_verify_reduce_segments: log_n outside 3..28");
  if (segment == 0) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "bp_verify_reduce_segments: segment is 0");
  if (!weights && m > 1 && segment != 1)
    return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "bp_verify_reduce_segments: weights may be NULL only where every segment is a single proof");
  if (n_public > ((size_t)1 << log_n)) return BP_FAIL(ctx, BP_ERR_LENGTH, "bp_verify_reduce_segments: more public inputs than rows");
  if (m >= (((size_t)1 << 31) - VERIFY_SHARED + VERIFY_POINTS - 1) / VERIFY_POINTS)
    return BP_FAIL(ctx, BP_ERR_TOO_LARGE, "bp_verify_reduce_segments: 9 m + 9 >= 2^31 points");
  if (first_bad) *first_bad = SIZE_MAX;
  for (float& v : ctx->verify_ms) v = 0;
  for (float& v : ctx->verify_seg_ms) v = 0;
  if (m == 0) return BP_OK;
  DeviceGuard guard(ctx->device);
  return verify_segments_run(ctx, log_n, vk768, proofs624, m, public_inputs, n_public, weights, challenges, scalar_fmt, segment, out192, first_bad);
}

int bp_verify_last_stats(bp_ctx* ctx, float stage_ms[5]) {
  if (!ctx || !stage_ms) return BP_ERR_INVALID_ARG;
  for (int k = 0; k < 5; k++) stage_ms[k] = ctx->verify_ms[k];
  return BP_OK;
}

int bp_verify_segments_last_stats(bp_ctx* ctx, float split_ms[3]) {
  if (!ctx || !split_ms) return BP_ERR_INVALID_ARG;
  for (int k = 0; k < 3; k++) split_ms[k] = ctx->verify_seg_ms[k];
  return BP_OK;
}

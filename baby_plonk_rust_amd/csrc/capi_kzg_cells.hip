// capi_kzg_cells.hip -- C ABI, part 9c: m cell claims (C_i, k_i, v_{i,0..l-1}, pi_i) of bp_kzg_open_cosets reduced to the two G1 points
// whose pairings decide them (bp_kzg_verify_cells_reduce).  With a_k = omega^(k l) and c_{i,t} the coefficients of the interpolant of
// claim i on its coset (kzg_open_cosets.hpp has the cells):
//   A = sum_i rho_i pi_i          B = sum_i rho_i (C_i + a_{k_i} pi_i) - sum_{t<l} (sum_i rho_i c_{i,t}) P_t
// and the batch holds iff pairing(A, [tau^l]_2) == pairing(B, G2).  Per claim the host computes two scalars (rho_i a_{k_i} and
// omega^(-k_i)); the device runs ONE batched inverse Fr transform of the m value rows (ntt.hip), kzg_cells_combine (kzg_kernels.hpp)
// and two MSMs (msm.hip); decoding and the subgroup test are the SRS loader's, as in bp_kzg_verify_reduce.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx.hpp"
#include "g1_check.hpp"
#include "g1_ntt.hpp"

#include "capi_common.hpp"

using namespace bp;

constexpr size_t NTT_BATCH_STEP = 32768;                 // ntt_run takes fewer than 65536 transforms at once

static int cells_reduce_run(bp_ctx* ctx, uint64_t srs, uint32_t log_l, const uint8_t* commitments96, const uint8_t* proofs96, size_t m,
                            const fr_t* vals, const fr_t* sc_head, const fr_t* w, uint32_t checks, uint8_t out192[192], size_t* first_bad) {
  const size_t l = (size_t)1 << log_l, n_claim = 2 * m, n_all = n_claim + l;      // C_i | pi_i | P_0 .. P_{l-1}
  uint8_t* d_bytes;
  g1_affine* d_pts;
  g1_affine28* d_p28;
  fr_t *d_sc, *d_vals, *d_w;                                                   // d_sc: rho_i | rho_i a_{k_i} | the l sums | rho_i again (A's)
  BP_TRY(ws_get(ctx, "kzg.v_bytes", n_claim * 96, (void**)&d_bytes));
  BP_TRY(ws_get(ctx, "kzg.v_points", n_all * sizeof(g1_affine), (void**)&d_pts));
  BP_TRY(ws_get(ctx, "kzg.v_p28", n_all * sizeof(g1_affine28), (void**)&d_p28));
  BP_TRY(ws_get(ctx, "kzg.v_scalars", (n_all + m) * sizeof(fr_t), (void**)&d_sc));
  BP_TRY(ws_get(ctx, "kzg.vc_values", m * l * sizeof(fr_t), (void**)&d_vals));
  BP_TRY(ws_get(ctx, "kzg.vc_w", m * sizeof(fr_t), (void**)&d_w));
  hipEvent_t* ev;
  BP_TRY(ev_get(ctx, "kzg", 5, hipEventDefault, &ev));
  hipStream_t st = ctx->stream;
  StreamDrain drain{st};                                                       // the uploads read the caller's and this call's pageable memory
  BP_HIP(ctx, hipEventRecord(ev[3], st));
  BP_HIP(ctx, hipMemcpyAsync(d_bytes, commitments96, m * 96, hipMemcpyHostToDevice, st));
  BP_HIP(ctx, hipMemcpyAsync(d_bytes + m * 96, proofs96, m * 96, hipMemcpyHostToDevice, st));
  BP_HIP(ctx, hipMemcpyAsync(d_sc, sc_head, n_claim * sizeof(fr_t), hipMemcpyHostToDevice, st));
  BP_HIP(ctx, hipMemcpyAsync(d_sc + n_all, sc_head, m * sizeof(fr_t), hipMemcpyHostToDevice, st));
  BP_HIP(ctx, hipMemcpyAsync(d_vals, vals, m * l * sizeof(fr_t), hipMemcpyHostToDevice, st));
  BP_HIP(ctx, hipMemcpyAsync(d_w, w, m * sizeof(fr_t), hipMemcpyHostToDevice, st));
  // P_0 .. P_{l-1}: from the shard(s) that hold them (a group: copied to the primary device, as bp_srs_lagrange collects its points)
  std::vector<SrsShard> sh;
  BP_TRY(srs_shards(ctx, srs, &sh, 0, l));
  for (const SrsShard& s : sh) {
    if (s.lo >= s.hi) continue;
    const g1_affine* part = s.e->d_points + (s.lo - s.e->first);
    const size_t bytes = (s.hi - s.lo) * sizeof(g1_affine);
    if (!peer_path(s.m, ctx->device)) BP_HIP(ctx, hipMemcpyAsync(d_pts + n_claim + s.lo, part, bytes, hipMemcpyDeviceToDevice, st));
    else BP_HIP(ctx, hipMemcpyPeerAsync(d_pts + n_claim + s.lo, ctx->device, part, s.m->device, bytes, st));
  }
  if (srs_decode_run(ctx, d_bytes, n_claim, d_pts) != BP_OK) {
    // the decoder says that a record was refused, not which: the rare path looks on the host, claim by claim
    g1_affine pt;
    for (size_t i = 0; i < m; i++) {
      if (host_point96(pt, proofs96 + 96 * i) && host_point96(pt, commitments96 + 96 * i)) continue;
      if (first_bad) *first_bad = i;
      char msg[120];
      snprintf(msg, sizeof msg, "claim %llu: a point was rejected (encoding, flags or not on the curve)", (unsigned long long)i);
      return BP_FAIL(ctx, BP_ERR_BAD_POINT, msg);
    }
    return BP_ERR_BAD_POINT;                                                   // the decoder's own message stands
  }
  if (checks & 1) {
    uint64_t bad_c = ~0ull, bad_w = ~0ull;
    BP_TRY(srs_subgroup_run(ctx, d_pts, m, &bad_c));
    BP_TRY(srs_subgroup_run(ctx, d_pts + m, m, &bad_w));
    size_t claim = SIZE_MAX;
    if (bad_c != ~0ull) claim = (size_t)(bad_c >> 2);
    if (bad_w != ~0ull) claim = std::min(claim, (size_t)(bad_w >> 2));
    if (claim != SIZE_MAX) {
      if (first_bad) *first_bad = claim;
      char msg[120];
      snprintf(msg, sizeof msg, "claim %llu: a point is not in the prime-order subgroup", (unsigned long long)claim);
      return BP_FAIL(ctx, BP_ERR_BAD_POINT, msg);
    }
  }
  // the interpolants: row i <- l^-1 sum_j v_ij zeta^(-j t) (one batched inverse transform), then the weighted sums per t
  if (log_l)
    for (size_t at = 0; at < m; at += NTT_BATCH_STEP)
      BP_TRY(ntt_run(ctx, d_vals + at * l, log_l, 1, std::min(NTT_BATCH_STEP, m - at), l));
  BP_TRY(kzg_cells_combine_run(ctx, d_vals, d_w, d_sc, m, log_l, d_sc + n_claim));
  BP_TRY(srs_to28_into(ctx, d_pts, n_all, d_p28));
  g1_proj A, B;
  BP_TRY(msm_run(ctx, d_p28, n_all, d_sc, BP_FR_MONT, 0, 0, &B));
  BP_TRY(msm_run(ctx, d_p28 + m, m, d_sc + n_all, BP_FR_MONT, 0, 0, &A));
  BP_HIP(ctx, hipEventRecord(ev[4], st));
  BP_HIP(ctx, stream_wait(st));
  BP_HIP(ctx, hipEventElapsedTime(&ctx->kzg_ms[2], ev[3], ev[4]));
  host_encode96(out192, A);
  host_encode96(out192 + 96, B);
  return BP_OK;
}

int bp_kzg_verify_cells_reduce(bp_ctx* ctx, uint64_t srs_handle, uint32_t log_n, uint32_t log_l, const uint8_t* commitments96, const uint32_t* cell_index,
                               const void* values, const uint8_t* proofs96, size_t m, const void* weights_or_null, int scalar_fmt, uint32_t checks,
                               uint8_t out192[192], size_t* first_bad) {
  if (!ctx || !out192 || !fmt_ok(scalar_fmt) || (m && (!commitments96 || !cell_index || !values || !proofs96))) return BP_ERR_INVALID_ARG;
  SrsEntry* e = nullptr;
  BP_TRY(srs_find(ctx, srs_handle, &e));
  if (e->basis != BP_BASIS_MONOMIAL) return BP_FAIL(ctx, BP_ERR_BASIS, "bp_kzg_verify_cells_reduce: the SRS must be powers of tau, not a Lagrange SRS");
  if (log_l > log_n) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "bp_kzg_verify_cells_reduce: log_l > log_n (a cell larger than the domain)");
  if (log_n >= G1_NTT_MAX_LOG) return BP_FAIL(ctx, BP_ERR_TOO_LARGE, "bp_kzg_verify_cells_reduce: log_n >= 24");
  const size_t l = (size_t)1 << log_l, r = (size_t)1 << (log_n - log_l);
  if (l > e->n_global) return BP_FAIL(ctx, BP_ERR_LENGTH, "bp_kzg_verify_cells_reduce: the SRS has fewer than l points");
  if (!weights_or_null && m > 1) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "bp_kzg_verify_cells_reduce: weights may be NULL for a single claim only");
  if (m >= ((size_t)1 << 30) / l) return BP_FAIL(ctx, BP_ERR_TOO_LARGE, "bp_kzg_verify_cells_reduce: m l >= 2^30 values");
  if (first_bad) *first_bad = SIZE_MAX;
  ctx->kzg_ms[2] = 0;
  if (m == 0) {
    encode_identity_pair(out192);
    return BP_OK;
  }
  // per claim on the host: the index, the values (Montgomery), rho_i, rho_i a_{k_i} and omega^(-k_i)
  std::vector<fr_t> vals(m * l), head(2 * m), w(m);
  const uint8_t *vb = (const uint8_t*)values, *rb = (const uint8_t*)weights_or_null;
  fr_t omega, omega_inv, omega_l;
  (void)host_root_of_unity(omega, (uint64_t)1 << log_n);
  fr_invert(omega_inv, omega);
  omega_l = fr_pow_u64(omega, (uint64_t)l);
  for (size_t i = 0; i < m; i++) {
    if (cell_index[i] >= r) {
      if (first_bad) *first_bad = i;
      char msg[96];
      snprintf(msg, sizeof msg, "claim %llu: the cell index is not below n / l", (unsigned long long)i);
      return BP_FAIL(ctx, BP_ERR_INVALID_ARG, msg);
    }
    bool ok = true;
    for (size_t j = 0; j < l && ok; j++) ok = fr_from_bytes(vals[i * l + j], vb + 32 * (i * l + j), scalar_fmt);
    head[i] = Fr::one();
    if (ok && rb) ok = fr_from_bytes(head[i], rb + 32 * i, scalar_fmt);
    if (!ok) {
      if (first_bad) *first_bad = i;
      char msg[96];
      snprintf(msg, sizeof msg, "claim %llu: a scalar is not canonical (>= q)", (unsigned long long)i);
      return BP_FAIL(ctx, BP_ERR_BAD_SCALAR, msg);
    }
    Fr::mul(head[m + i], head[i], fr_pow_u64(omega_l, cell_index[i]));
    w[i] = fr_pow_u64(omega_inv, cell_index[i]);
  }
  DeviceGuard guard(ctx->device);
  return cells_reduce_run(ctx, srs_handle, log_l, commitments96, proofs96, m, vals.data(), head.data(), w.data(), checks, out192, first_bad);
}

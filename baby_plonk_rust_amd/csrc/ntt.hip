// ntt.hip -- host driver of the Fr NTT: twiddle tables, the knobs, and one launcher per kernel (kernels in ntt_kernels.hpp; every
// shape comes from the plan of ntt_plan.hpp).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ctx.hpp"
#include "ntt_kernels.hpp"

namespace bp {

static fr_t host_root_pow2(bool inverse, uint32_t log_order) {
  // w_{2^log_order} = ROOT_OF_UNITY^(2^(32 - log_order))   (utils.rs:39-43)
  fr_t w = fr_root_of_unity(inverse);
  for (uint32_t i = log_order; i < 32; i++) Fr::sqr(w, w);
  return w;
}

static int make_table(bp_ctx* ctx, const fr_t& base, uint32_t count, uint32_t shift, const fr_t* d_scale, fr_t* d_out_fr,
                      tw29_t* d_out_tw) {
  hipLaunchKernelGGL(ntt_make_table, dim3((count + 255) / 256), dim3(256), 0, ctx->stream, base, count, shift, d_scale, d_out_fr,
                     d_out_tw);
  BP_HIP(ctx, hipGetLastError());
  return BP_OK;
}

int ntt_init_tables(bp_ctx* ctx) {
  for (int inv = 0; inv < 2; inv++) {
    BP_HIP(ctx, hipMalloc((void**)&ctx->small_tw[inv], 512 * sizeof(tw29_t)));
    BP_TRY(make_table(ctx, host_root_pow2(inv != 0, NTT_SMALL_MAX_LOG), 512, 0, nullptr, nullptr, ctx->small_tw[inv]));
  }
  // per function and per device: set for every context (this runs in bp_init, after hipSetDevice)
  BP_HIP(ctx, hipFuncSetAttribute((const void*)ntt_small, hipFuncAttributeMaxDynamicSharedMemorySize, NTT_PAD_LDS_MAX));
  BP_HIP(ctx, hipFuncSetAttribute((const void*)ntt_pass_strided, hipFuncAttributeMaxDynamicSharedMemorySize, NTT_PAD_LDS_MAX));
  BP_HIP(ctx, hipFuncSetAttribute((const void*)ntt_pass_last, hipFuncAttributeMaxDynamicSharedMemorySize, NTT_PAD_LDS_MAX));
  BP_HIP(ctx, hipFuncSetAttribute((const void*)ntt_pass_strided_swz, hipFuncAttributeMaxDynamicSharedMemorySize, NTT_SWZ_LDS_MAX));
  BP_HIP(ctx, hipFuncSetAttribute((const void*)ntt_pass_last_swz, hipFuncAttributeMaxDynamicSharedMemorySize, NTT_SWZ_LDS_MAX));
  return BP_OK;
}

// the BP_NTT_* knobs, read on every call (a test may change one between two transforms); the shipped build reads nothing: knob()
// is nullptr there and the defaults of NttKnobs stand
NttKnobs ntt_knobs() {
  NttKnobs kn;
  static const char* const cols[4] = {"BP_NTT_COLS_LOG_L7", "BP_NTT_COLS_LOG_L8", "BP_NTT_COLS_LOG_L9", "BP_NTT_COLS_LOG_L10"};
  kn.three_pass_from = knob_u32("BP_NTT_THREE_PASS_FROM", kn.three_pass_from, 11, 29);
  for (int i = 0; i < 4; i++) kn.cols_log[i] = knob_u32(cols[i], kn.cols_log[i], 0, 3);
  kn.swizzle = knob_u32("BP_NTT_SWIZZLE", kn.swizzle, 0, 1);
  kn.lanes_shift = knob_u32("BP_NTT_LANES_SHIFT", kn.lanes_shift, 0, 1);
  kn.full_twiddles_max_log = knob_u32("BP_NTT_FULL_TWIDDLES_MAX_LOG", kn.full_twiddles_max_log, 0, 28);
  kn.group_split_from = knob_u32("BP_NTT_GROUP_SPLIT_FROM", kn.group_split_from, 11, 29);
  if (const char* e = knob("BP_NTT_SPLIT")) {
    unsigned kk = 0, w[3] = {0, 0, 0};
    if (sscanf(e, "%u:%u,%u,%u", &kk, &w[0], &w[1], &w[2]) >= 3) {
      kn.split_k = kk;
      for (int i = 0; i < 3; i++) kn.split_l[i] = w[i];
    }
  }
  return kn;
}

static int get_tables(bp_ctx* ctx, uint32_t k, int inverse, NttTables** out) {
  const uint32_t key = k * 2 + (inverse ? 1 : 0);
  auto it = ctx->ntt_tables.find(key);
  if (it != ctx->ntt_tables.end()) {
    *out = &it->second;
    return BP_OK;
  }
  NttTables t;
  t.h = (k + 1) / 2;
  const uint32_t nlo = 1u << t.h, nhi = 1u << (k - t.h);
  const fr_t w = host_root_pow2(inverse != 0, k);
  BP_HIP(ctx, hipMalloc((void**)&t.lo, (size_t)nlo * sizeof(tw29_t)));
  BP_HIP(ctx, hipMalloc((void**)&t.hi, (size_t)nhi * sizeof(tw29_t)));
  BP_TRY(make_table(ctx, w, nlo, 0, nullptr, nullptr, t.lo));
  BP_TRY(make_table(ctx, w, nhi, t.h, nullptr, nullptr, t.hi));
  if (inverse) {
    const fr_t n_inv = finv(fr_from_u64((uint64_t)1 << k));     // N^-1 in Montgomery form (utils.rs:126: Scalar::from(n).invert())
    BP_HIP(ctx, hipMalloc((void**)&t.n_inv, sizeof(fr_t)));
    BP_HIP(ctx, hipMemcpyAsync(t.n_inv, &n_inv, sizeof(fr_t), hipMemcpyHostToDevice, ctx->stream));
    BP_HIP(ctx, stream_wait(ctx->stream));    // n_inv lives on this stack frame
    BP_HIP(ctx, hipMalloc((void**)&t.hi_scaled, (size_t)nhi * sizeof(tw29_t)));
    BP_TRY(make_table(ctx, w, nhi, t.h, t.n_inv, nullptr, t.hi_scaled));
    BP_HIP(ctx, hipMalloc((void**)&t.n_inv_tw, sizeof(tw29_t)));
    BP_TRY(make_table(ctx, w, 1, 0, t.n_inv, nullptr, t.n_inv_tw));       // w^0 * N^-1
  }
  ctx->ntt_tables[key] = t;
  *out = &ctx->ntt_tables[key];
  return BP_OK;
}

int ntt_tmp_buffer(bp_ctx* ctx, uint32_t k, fr_t** out) { return ws_get(ctx, "ntt.tmp", ((size_t)1 << k) * sizeof(fr_t), (void**)out); }

// what one ntt_run_part hands its launchers
struct NttRun {
  bp_ctx* ctx;
  const NttHostPlan& plan;
  NttTables* tab;
  fr_t *data, *tmp;          // ping-pong: pass 1 data -> tmp, middle passes in tmp, last pass tmp -> data
  int inverse;
  size_t batch, stride;
  const tw29_t* small_tw() const { return ctx->small_tw[inverse ? 1 : 0]; }
  size_t N() const { return (size_t)1 << plan.dev.k; }
};
struct TileRange { unsigned first, count; };
// the part's share of a pass's tiles (phase < 0: all of them)
static TileRange tile_share(unsigned tiles, int phase, uint32_t part, uint32_t parts) {
  return phase < 0 ? TileRange{0u, tiles} : TileRange{tiles / parts * part, tiles / parts};
}
static const tw29_t* pass_hi(const NttTables* tab, uint32_t i, int inverse) {
  return (inverse && i == 0) ? tab->hi_scaled : tab->hi;   // N^-1 rides on the first twiddle
}

// tab->full[i], the full inter-pass twiddle table of strided pass i (nullptr: the drain uses the two-level lookup); built once per
// (N, direction, pass), and again when a knob changed the split since
static int pass_table(bp_ctx* ctx, NttTables* tab, const NttHostPlan& plan, uint32_t i, int inverse, const tw29_t** out) {
  const uint32_t l = plan.pass[i].l, s = plan.pass[i].s, ls = (l << 8) | s;
  if (tab->full[i] && tab->full_ls[i] != ls) {
    BP_HIP(ctx, stream_wait(ctx->stream));
    BP_HIP(ctx, hipFree(tab->full[i]));
    tab->full[i] = nullptr;
  }
  if (!tab->full[i] && plan.full_tables) {
    const size_t M = (size_t)1 << (l + s);
    tab->full_ls[i] = ls;
    BP_HIP(ctx, hipMalloc((void**)&tab->full[i], M * sizeof(tw29_t)));
    hipLaunchKernelGGL(ntt_make_pass_table, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, ctx->stream, tab->lo, pass_hi(tab, i, inverse), tab->h,
                       l, s, plan.dev.k - (l + s), tab->full[i]);
    BP_HIP(ctx, hipGetLastError());
  }
  *out = tab->full[i];
  return BP_OK;
}

static void launch_small(const NttRun& r) {
  const NttPass& p = r.plan.pass[0];
  hipLaunchKernelGGL(ntt_small, dim3((unsigned)r.batch), dim3(p.threads), p.lds_bytes, r.ctx->stream, r.data, r.stride, r.plan.dev.k, r.small_tw(),
                     r.inverse ? r.tab->n_inv_tw : (const tw29_t*)nullptr);
}
static int launch_strided(const NttRun& r, uint32_t i, TileRange tiles) {
  const NttPass& p = r.plan.pass[i];
  const tw29_t* full;
  BP_TRY(pass_table(r.ctx, r.tab, r.plan, i, r.inverse, &full));
  NttStridedArgs sa;
  sa.src = i == 0 ? (const fr_t*)r.data : (const fr_t*)r.tmp;
  sa.src_stride = i == 0 ? r.stride : r.N();
  sa.k = r.plan.dev.k; sa.l = p.l; sa.s = p.s; sa.cl = p.cl;
  sa.small_tw = r.small_tw();
  sa.tile0 = tiles.first;
  sa.h = r.tab->h;
  sa.dst = (decltype(sa.dst))r.tmp;
  sa.dst_stride = r.N();
  sa.tw_lo = (decltype(sa.tw_lo))r.tab->lo; sa.tw_hi = (decltype(sa.tw_hi))pass_hi(r.tab, i, r.inverse); sa.tw_full = (decltype(sa.tw_full))full;
  hipLaunchKernelGGL(p.swizzled ? ntt_pass_strided_swz : ntt_pass_strided, dim3(tiles.count, (unsigned)r.batch), dim3(p.threads), p.lds_bytes,
                     r.ctx->stream, sa);
  return BP_OK;
}
static void launch_last(const NttRun& r, TileRange tiles) {
  const NttPass& p = r.plan.pass[r.plan.dev.P - 1];
  NttLastArgs la;
  la.src = r.tmp;
  la.src_stride = r.N();
  la.small_tw = r.small_tw();
  la.tile0 = tiles.first;
  la.plan = r.plan.dev;
  la.dst = (decltype(la.dst))r.data;
  la.dst_stride = r.stride;
  hipLaunchKernelGGL(p.swizzled ? ntt_pass_last_swz : ntt_pass_last, dim3(tiles.count, (unsigned)r.batch), dim3(p.threads), p.lds_bytes,
                     r.ctx->stream, la);
}

// phase -1: the whole transform; 0 / 1: the two phases of a transform cut over `parts` members (ntt_split_ok; batch must be 1)
int ntt_run_part(bp_ctx* ctx, const NttHostPlan& plan, fr_t* d_data, int inverse, size_t batch, size_t stride, int phase, uint32_t part,
                 uint32_t parts) {
  const uint32_t k = plan.dev.k, P = plan.dev.P;
  if (k > 28) return BP_FAIL(ctx, BP_ERR_TOO_LARGE, "NTT length > 2^28");
  if (batch == 0) return BP_OK;
  if (batch > 65535) return BP_FAIL(ctx, BP_ERR_TOO_LARGE, "NTT batch > 65535");
  const size_t N = (size_t)1 << k;
  if (batch > 1 && stride < N) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "NTT stride < N");
  if (phase >= 0 && (batch != 1 || !ntt_split_ok(plan, parts) || part >= parts)) return BP_FAIL(ctx, BP_ERR_INVALID_ARG, "NTT phase");
  NttRun r = {ctx, plan, nullptr, d_data, nullptr, inverse, batch, stride};
  BP_TRY(get_tables(ctx, k, inverse, &r.tab));
  BP_HIP(ctx, hipEventRecord(ctx->ev[phase == 1 ? 2 : 0], ctx->stream));
  if (P == 1) {
    launch_small(r);
  } else {
    BP_TRY(ws_get(ctx, "ntt.tmp", batch * N * sizeof(fr_t), (void**)&r.tmp));
    for (uint32_t i = 0; i + 1 < P; i++) {
      if ((phase == 0 && i > 0) || (phase == 1 && i == 0)) continue;
      BP_TRY(launch_strided(r, i, tile_share(plan.pass[i].tiles, phase, part, parts)));
    }
    if (phase != 0) launch_last(r, tile_share(plan.pass[P - 1].tiles, phase, part, parts));
  }
  BP_HIP(ctx, hipGetLastError());
  BP_HIP(ctx, hipEventRecord(ctx->ev[phase == 1 ? 3 : 1], ctx->stream));
  ctx->ntt_passes = P;
  return BP_OK;
}
int ntt_run(bp_ctx* ctx, fr_t* d_data, uint32_t k, int inverse, size_t batch, size_t stride) {
  return ntt_run_part(ctx, ntt_plan(k, ntt_knobs()), d_data, inverse, batch, stride, -1, 0, 1);
}

// out[j] = w^j, j < n   (roots_of_unity, utils.rs:45-52)
int roots_run(bp_ctx* ctx, const fr_t& w, size_t n, fr_t* d_out) {
  if (n == 0) return BP_OK;
  return make_table(ctx, w, (uint32_t)n, 0, nullptr, d_out, nullptr);
}

}  // namespace bp

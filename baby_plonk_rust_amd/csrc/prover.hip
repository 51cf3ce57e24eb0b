// prover.hip -- Prover::prove (src/prover.rs:64-175; rounds 1-5 :177-647) on the GPU behind the C ABI, with the eleven
// blinding scalars as an input (the reference draws them from thread_rng, :108-110, so its proofs are not reproducible)
// and the Fiat-Shamir challenges from the host transcript (transcript.hpp, src/transcript.rs:4-86).
//
// The reference builds every round out of value-semantics `Polynomial` operators (each product = three O(n^2) DFTs,
// each division a long division).  Every committed or evaluated polynomial is uniquely determined by the witness, the
// circuit, the blinders and the challenges, so this file computes the same polynomials by the cheapest exact route:
//   round 1/2  b(x) (x^n - 1) + iNTT(values) written directly (fr_blind); grand product by scans (poly_kernels.hpp);
//   round 3    the quotient t = (gate + alpha perm + alpha^2 first_row) / (x^n - 1) point-wise on the coset g <w_4n>
//              (5 coset NTTs of the witness polynomials + 1 inverse; the circuit's 9 coset columns are cached);
//   round 5    the opening numerator as one fused linear combination, division by x - zeta as a scan (poly.hip).
// The reference's Div squeezes zero quotient coefficients out (polynomial.rs:371-376); the same compaction is applied
// wherever a quotient has one (probability ~ deg / q with random blinders).
// Host arithmetic on numbers alone (the coset's constants, the choice of path, the scalars of rounds 3 and 5): prover_host.hpp.
// Parity: tests/test_native_prover.py -- proof bytes equal the reference-shaped restatement (tests/prover_rounds.py) run
// on the CPU oracle, and the committed golden proof of the toy circuit (tests/verify_proof_test.rs).
#include <string.h>

#include <algorithm>
#include <chrono>

#include "ctx.hpp"
#include "prover_kernels.hpp"
#include "transcript.hpp"

namespace bp {

namespace {

constexpr int N_PRE = 9;                 // ql qr qm qo qc s1 s2 s3 (+ L1 on the coset)
unsigned blocks_of(size_t threads) { return (unsigned)((threads + 255) / 256); }
fr_t omega_of(uint32_t log_n) { fr_t w; (void)host_root_of_unity(w, (uint64_t)1 << log_n); return w; }      // w_n (prover.rs:99)
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// (numerator of na coefficients) / (x - point) -> d_q, *nq coefficients, by the reference's Div semantics
int divide_by_linear(bp_ctx* ctx, fr_t* d_num, size_t na, const fr_t& point, fr_t* d_q, size_t* nq) {
  size_t na_eff;
  BP_TRY(fr_nonzero_stats_run(ctx, d_num, na, 0, 0, &na_eff, nullptr));              // trailing zeros trimmed (polynomial.rs:325-339)
  *nq = 0;
  if (na_eff < 2) return BP_OK;
  fr_t* d_b;
  BP_TRY(ws_get(ctx, "prove.divisor", 2 * sizeof(fr_t), (void**)&d_b));
  const fr_t hb[2] = {fneg(point), Fr::one()};
  BP_HIP(ctx, hipMemcpyAsync(d_b, hb, sizeof hb, hipMemcpyHostToDevice, ctx->stream));
  *nq = na_eff - 1;
  BP_TRY(poly_div_run(ctx, d_num, na_eff, d_b, 2, hb[0], hb[1], true, d_q, *nq));
  return fr_squeeze_zeros_run(ctx, d_q, nq);
}

// ---- evaluation on the quotient coset g <w_4n>: out[i] = coef[i] g^i, zero-padded to 4n, is what the size-4n transform takes
void coset_shift_pad(hipStream_t st, const CircuitEntry& cir, const fr_t* coef, size_t len, fr_t* out) {
  const size_t N = (size_t)4 << cir.log_n;
  hipLaunchKernelGGL(fr_mul_table_pad, dim3(blocks_of(N)), dim3(256), 0, st, coef, len, cir.g_pow, out, N);
}
// f(first, count) for every contiguous run of the slots (a, b, c, z, PI) that `which` selects: a run is transformed as one batch
template <class F>
int for_each_run(unsigned which, F f) {
  for (int p = 0, q; p < 5; p = q + 1) {
    for (q = p; q < 5 && (which >> q & 1);) q++;      // slots [p, q) are selected, q is not
    if (q > p) BP_TRY(f(p, q - p));
  }
  return BP_OK;
}
// ev[slot] (4n each) = the evaluations of the selected coefficient vectors, on on's stream; pi_zero: PI(X) = 0, its slot is zeroed
int coset_eval(bp_ctx* on, const CircuitEntry& cir, const fr_t* const coefs5[5], const size_t lens5[5], unsigned which, bool pi_zero, fr_t* ev) {
  const size_t N = (size_t)4 << cir.log_n;
  for (int p = 0; p < 5; p++)
    if (which >> p & 1) coset_shift_pad(on->stream, cir, coefs5[p], lens5[p], ev + (size_t)p * N);
  if (pi_zero) BP_HIP(on, hipMemsetAsync(ev + 4 * N, 0, N * sizeof(fr_t), on->stream));
  BP_HIP(on, hipGetLastError());
  return for_each_run(which, [&](int p, int cnt) { return ntt_run(on, ev + (size_t)p * N, cir.log_n + 2, 0, (size_t)cnt, N); });
}

}  // namespace

ProvePaths prove_paths_of(const bp_ctx* ctx, const CircuitEntry& cir, bool host_witness) {      // the one reader of the four knobs
  const ProveKnobs knobs = {knob_tristate(knob("BP_PROVE_STAGED")), knob_tristate(knob("BP_PROVE_COSET_SPLIT")), knob_tristate(knob("BP_PROVE_SIDE")),
                            knob_tristate(knob("BP_PROVE_COSET_EARLY"))};
  return prove_paths(cir.log_n, host_witness, is_group(ctx), !cir.split.empty(), knobs);
}

// ------------------------------------------------------------------------------------------------ circuit
static int circuit_fill(bp_ctx* ctx, const fr_t* d_lag, CircuitEntry& e) {
  const uint32_t log_n = e.log_n;
  const size_t n = (size_t)1 << log_n, N = 4 * n;
  BP_HIP(ctx, hipMalloc((void**)&e.coef, 8 * n * sizeof(fr_t)));
  BP_HIP(ctx, hipMalloc((void**)&e.coset, (size_t)N_PRE * N * sizeof(fr_t)));
  BP_HIP(ctx, hipMalloc((void**)&e.coset_x, N * sizeof(fr_t)));
  BP_HIP(ctx, hipMalloc((void**)&e.g_pow, (n + 8) * sizeof(fr_t)));
  BP_HIP(ctx, hipMalloc((void**)&e.roots, n * sizeof(fr_t)));
  BP_HIP(ctx, hipMalloc((void**)&e.ginv_pow, N * sizeof(fr_t)));
  BP_TRY(roots_run(ctx, e.cc.g, n + 8, e.g_pow));
  BP_TRY(roots_run(ctx, omega_of(log_n), n, e.roots));
  BP_TRY(roots_run(ctx, e.cc.ginv, N, e.ginv_pow));
  BP_TRY(roots_run(ctx, e.cc.w4n, N, e.coset_x));                                        // w_4n^i ...
  BP_TRY(fr_scalar_run(ctx, e.coset_x, e.cc.g, e.coset_x, N, 2));                       // ... times g
  // coefficient forms (prover.rs:379-386 recomputes these i_ntt's in every proof)
  BP_HIP(ctx, hipMemcpyAsync(e.coef, d_lag, 8 * n * sizeof(fr_t), hipMemcpyDeviceToDevice, ctx->stream));
  BP_TRY(ntt_run(ctx, e.coef, log_n, 1, 8, n));
  // their evaluations on the quotient coset, and L1's (l1_coeff = i_ntt(e_0) = [1/n; n], prover.rs:430)
  for (int k = 0; k < 8; k++) coset_shift_pad(ctx->stream, e, e.coef + (size_t)k * n, n, e.coset + (size_t)k * N);
  fr_t* l1;
  BP_TRY(ws_get(ctx, "prove.l1", n * sizeof(fr_t), (void**)&l1));
  BP_HIP(ctx, hipMemsetAsync(l1, 0, n * sizeof(fr_t), ctx->stream));
  BP_TRY(fr_scalar_run(ctx, l1, e.cc.n_inv, l1, n, 0));                                  // 0 + 1/n
  coset_shift_pad(ctx->stream, e, l1, n, e.coset + (size_t)8 * N);
  BP_HIP(ctx, hipGetLastError());
  return ntt_run(ctx, e.coset, log_n + 2, 0, N_PRE, N);
}
// takes ownership of d_lag only on success
int circuit_build(bp_ctx* ctx, uint32_t log_n, fr_t* d_lag, CircuitEntry* out) {
  CircuitEntry e;
  e.log_n = log_n;
  e.cc = coset_consts(log_n);
  int rc = circuit_fill(ctx, d_lag, e);
  if (rc == BP_OK && stream_wait(ctx->stream) != hipSuccess) rc = fail(ctx, BP_ERR_HIP, "circuit_build", hipGetLastError(), __FILE__, __LINE__);
  if (rc != BP_OK) {
    circuit_release(e);               // e.lag is still null: the caller keeps d_lag
    return rc;
  }
  e.lag = d_lag;
  *out = e;
  return BP_OK;
}
void circuit_release(CircuitEntry& e) {
  fr_t** owned[7] = {&e.lag, &e.coef, &e.coset, &e.coset_x, &e.g_pow, &e.ginv_pow, &e.roots};
  for (fr_t** p : owned) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
  if (e.sigma_target) (void)hipFree(e.sigma_target);
  e.sigma_target = nullptr;
  if (e.wire_ids) (void)hipFree(e.wire_ids);
  e.wire_ids = nullptr;
  for (CosetShare& sh : e.split) {
    DeviceGuard guard(sh.member ? sh.member->device : 0);
    if (sh.member) (void)hipStreamSynchronize(sh.member->stream);
    if (sh.work) (void)hipStreamSynchronize(sh.work->stream);        // the work context itself is the member's side context: destroyed with the member
    fr_t** mine[4] = {&sh.pre, &sh.xs, &sh.spow, &sh.sinv};
    for (fr_t** p : mine) {
      if (*p) (void)hipFree(*p);
      *p = nullptr;
    }
    if (sh.done) (void)hipEventDestroy(sh.done);
    sh.done = nullptr;
  }
  e.split.clear();
}

// ------------------------------------------------------------------------------------------------ round 3 by coset (group contexts)
// src (on device src_dev) -> dst (on m's device), n elements, on m's stream
// (owner: the group member the stream's context belongs to, when m is that member's side context)
static hipError_t copy_to_member(bp_ctx* m, fr_t* dst, const fr_t* src, int src_dev, size_t n, const bp_ctx* owner = nullptr) {
  if (!peer_path(owner ? owner : m, src_dev)) return hipMemcpyAsync(dst, src, n * sizeof(fr_t), hipMemcpyDeviceToDevice, m->stream);
  return hipMemcpyPeerAsync(dst, m->device, src, src_dev, n * sizeof(fr_t), m->stream);
}

// The members' coset shares of a circuit (leader of a group; called once per circuit).  Coset j of the four is entries 4 i + j of
// the leader's tables over g <w_4n>, so a share is gathered there (strided) and copied to its member; the s_j^i / s_j^-i tables are
// computed on the member.  The first 2 members (groups of 2 or 3) take two cosets each, the first 4 (groups of 4 and more) one.
int circuit_split_build(bp_ctx* ctx, CircuitEntry& e) {
  // experiment (BP_PROVE_COSET_ONE=1): ONE device takes all four cosets itself -- four size-n coset transforms per
  // polynomial instead of one zero-padded size-4n transform; measured in profiles/r06_round3_coset_one_gpu_ab.txt
  const bool one_gpu = ctx->members.size() < 2 && knob_u32("BP_PROVE_COSET_ONE", 0, 0, 1) == 1;
  const size_t R = one_gpu ? 1 : ctx->members.size();
  if (R < 2 && !one_gpu) return BP_OK;
  const size_t n = (size_t)1 << e.log_n, N = 4 * n;
  const uint32_t used = one_gpu ? 1 : (R >= 4 ? 4 : 2), per = 4 / used;
  fr_t* tmp;
  BP_TRY(ws_get(ctx, "prove.split_tmp", 10 * n * sizeof(fr_t), (void**)&tmp));
  for (uint32_t r = 0; r < used; r++) {
    CosetShare sh;
    bp_ctx* m = one_gpu ? ctx : ctx->members[r];
    sh.member = m, sh.first = r * per, sh.count = per;
    // a stream, workspace and transform tables of its own on the member's device: the share's work runs beside the member's MSM
    // shards instead of queueing behind them
    BP_TRY(lift(ctx, m, side_ctx_get(m, &sh.work)));
    {
      DeviceGuard guard(m->device);
      hipError_t he = hipMalloc((void**)&sh.pre, (size_t)per * 9 * n * sizeof(fr_t));
      if (he == hipSuccess) he = hipMalloc((void**)&sh.xs, (size_t)per * n * sizeof(fr_t));
      if (he == hipSuccess) he = hipMalloc((void**)&sh.spow, (size_t)per * n * sizeof(fr_t));
      if (he == hipSuccess) he = hipMalloc((void**)&sh.sinv, (size_t)per * n * sizeof(fr_t));
      if (he == hipSuccess) he = hipEventCreateWithFlags(&sh.done, hipEventDisableTiming);
      e.split.push_back(sh);                 // owned by the entry from here on (circuit_release frees what was allocated)
      if (he != hipSuccess) return fail(ctx, BP_ERR_HIP, "coset share", he, __FILE__, __LINE__);
    }
    for (uint32_t c = 0; c < per; c++) {
      const uint32_t j = sh.first + c;
      {                                       // gather coset j on the leader, wait, copy to the member
        DeviceGuard guard(ctx->device);
        for (int col = 0; col < N_PRE; col++)
          hipLaunchKernelGGL(fr_gather_stride, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, e.coset + (size_t)col * N, (size_t)4, (size_t)j, n, tmp + (size_t)col * n);
        hipLaunchKernelGGL(fr_gather_stride, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, e.coset_x, (size_t)4, (size_t)j, n, tmp + (size_t)N_PRE * n);
        BP_HIP(ctx, hipGetLastError());
        BP_HIP(ctx, stream_wait(ctx->stream));
      }
      DeviceGuard guard(m->device);
      BP_HIP(ctx, copy_to_member(m, sh.pre + (size_t)c * 9 * n, tmp, ctx->device, (size_t)N_PRE * n));
      BP_HIP(ctx, copy_to_member(m, sh.xs + (size_t)c * n, tmp + (size_t)N_PRE * n, ctx->device, n));
      BP_TRY(lift(ctx, m, roots_run(m, e.cc.s[j], n, sh.spow + (size_t)c * n)));
      BP_TRY(lift(ctx, m, roots_run(m, e.cc.s_inv[j], n, sh.sinv + (size_t)c * n)));
      BP_HIP(ctx, stream_wait(m->stream));    // tmp is reused for the next coset
    }
  }
  return BP_OK;
}

// what the five rounds of one proof share
struct Prove {
  bp_ctx* ctx;
  uint64_t srs;
  const CircuitEntry& cir;
  const fr_t *d_wit, *blind;                    // prove_run's arguments, as are proof, pi_zero, staged
  uint8_t* proof;
  bool pi_zero;
  const ProveStaged* staged;
  ProvePaths path;
  size_t n;
  fr_t omega;
  PlonkTranscript tr;
  g1_proj cm[9];
  fr_t *coefs, *abc[3], *z_lag, *z_coeff, *ev, *t, *t_part[3], *num, *w[2];      // workspaces (prove_workspaces)
  const fr_t* coefs5[5];                        // a, b, c, z, PI in coefficient form: the slots of coset_eval / coset_inputs ...
  size_t lens5[5], hi_len;                      // ... their lengths; coefficients of t_hi
  fr_t beta, gamma, alpha, zeta, nu, bar[6], pi_zeta;      // bar: a b c s1 s2 at zeta, z at zeta w (the proof's six evaluations)
  hipEvent_t* side_ev = nullptr;                // path.side: the context's two "side" events, taken by round 1: [0] inputs ready, [1] side work done
};

// Round 3 by coset, in two parts, both on the shares' work contexts (CosetShare::work).
//  early: a, b, c and PI depend on no challenge (prover.rs:386-450 evaluates them after alpha only because the reference is
//         sequential): the leader enqueues their copies, folds and size-n transforms right after round 1's blinding, so they run on
//         the members beside the commitments of rounds 1 and 2 -- the members' GPUs only hold an MSM shard each then.
//  late:  once z's coefficients exist, its copy / fold / transform, the quotient on each coset, the inverse transform, the
//         unscaling by s_j^-i and the copy of the n coefficients back to the leader, which recombines the four residues.
// slots: a, b, c, z, PI (the order quotient_coset reads); `which` selects the slots a call handles.
static int coset_inputs(const Prove& p, const CosetShare& sh, unsigned which, bool zero_pi, fr_t** ev_out) {
  bp_ctx *ctx = p.ctx, *w = sh.work;
  const uint32_t k = p.cir.log_n;
  const size_t n = p.n, cap = n + 8;
  fr_t *cf, *ev;
  BP_TRY(lift(ctx, w, ws_get(w, "prove.split_coef", 5 * cap * sizeof(fr_t), (void**)&cf)));
  BP_TRY(lift(ctx, w, ws_get(w, "prove.split_ev", (size_t)sh.count * 5 * n * sizeof(fr_t), (void**)&ev)));
  if (ev_out) *ev_out = ev;
  BP_HIP(ctx, hipStreamWaitEvent(w->stream, ctx->ev[4], 0));          // the coefficient vectors are ready behind the leader's event
  for (int s = 0; s < 5; s++)
    if (which >> s & 1) BP_HIP(ctx, copy_to_member(w, cf + (size_t)s * cap, p.coefs5[s], ctx->device, p.lens5[s], sh.member));
  for (uint32_t c = 0; c < sh.count; c++) {
    fr_t* e = ev + (size_t)c * 5 * n;
    if (zero_pi) BP_HIP(ctx, hipMemsetAsync(e + 4 * n, 0, n * sizeof(fr_t), w->stream));      // PI(X) = 0 on every coset
    for (int s = 0; s < 5; s++)
      if (which >> s & 1)
        hipLaunchKernelGGL(fr_fold_scale, dim3(blocks_of(n)), dim3(256), 0, w->stream, cf + (size_t)s * cap, p.lens5[s], n, p.cir.cc.sn[sh.first + c],
                           sh.spow + (size_t)c * n, e + (size_t)s * n);
    BP_HIP(ctx, hipGetLastError());
    BP_TRY(for_each_run(which, [&](int s, int cnt) { return lift(ctx, w, ntt_run(w, e + (size_t)s * n, k, 0, (size_t)cnt, n)); }));
  }
  return BP_OK;
}

// p.t (4n coefficients on the leader) = quotient of round 3.  With p.path.early, a, b, c, PI are already on the cosets.
static int round3_by_coset(const Prove& p) {
  bp_ctx* ctx = p.ctx;
  const size_t n = p.n;
  fr_t* v;                                                            // the four residues, one after the other
  BP_TRY(ws_get(ctx, "prove.split_v", 4 * n * sizeof(fr_t), (void**)&v));
  BP_HIP(ctx, hipEventRecord(ctx->ev[4], ctx->stream));              // z's coefficients (and the others, if not sent early) are ready behind this event
  for (const CosetShare& sh : p.cir.split) {
    bp_ctx* w = sh.work;
    DeviceGuard guard(w->device);
    fr_t *ev, *tq;
    BP_TRY(coset_inputs(p, sh, p.path.early ? 0x08u : (p.pi_zero ? 0x0Fu : 0x1Fu), p.pi_zero && !p.path.early, &ev));
    BP_TRY(lift(ctx, w, ws_get(w, "prove.split_tq", n * sizeof(fr_t), (void**)&tq)));
    for (uint32_t c = 0; c < sh.count; c++) {
      const uint32_t j = sh.first + c;
      const fr_t& z = p.cir.cc.zh_inv[j];
      const fr_t zh[4] = {z, z, z, z};                                   // X^n - 1 = s_j^n - 1 on the whole coset
      hipLaunchKernelGGL(quotient_coset, dim3(blocks_of(n)), dim3(256), 0, w->stream, ev + (size_t)c * 5 * n, sh.pre + (size_t)c * 9 * n, sh.xs + (size_t)c * n, n,
                         quotient_args(p.alpha, p.beta, p.gamma, zh), tq, 1u);
      BP_HIP(ctx, hipGetLastError());
      BP_TRY(lift(ctx, w, ntt_run(w, tq, p.cir.log_n, 1, 1, n)));
      BP_TRY(lift(ctx, w, fr_binary_run(w, tq, n, sh.sinv + (size_t)c * n, n, tq, n, 2)));      // coefficients of t mod (x^n - s_j^n)
      // back to the leader: the copy is issued on the work stream (it follows the kernels that produced tq)
      hipError_t he = !peer_path(sh.member ? sh.member : w, ctx->device)
                          ? hipMemcpyAsync(v + (size_t)j * n, tq, n * sizeof(fr_t), hipMemcpyDeviceToDevice, w->stream)
                          : hipMemcpyPeerAsync(v + (size_t)j * n, ctx->device, tq, w->device, n * sizeof(fr_t), w->stream);
      if (he != hipSuccess) return fail(ctx, BP_ERR_HIP, "coset quotient back to the leader", he, __FILE__, __LINE__);
    }
    BP_HIP(ctx, hipEventRecord(sh.done, w->stream));
  }
  DeviceGuard guard(ctx->device);
  for (const CosetShare& sh : p.cir.split) BP_HIP(ctx, hipStreamWaitEvent(ctx->stream, sh.done, 0));
  hipLaunchKernelGGL(coset_recombine, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, v, n, recombine_args(p.cir.cc), p.t);
  BP_HIP(ctx, hipGetLastError());
  return BP_OK;
}

// ------------------------------------------------------------------------------------------------ prove
static int prove_workspaces(Prove& p) {
  bp_ctx* ctx = p.ctx;
  const size_t n = p.n, pad = n + 8;
  fr_t *abc, *zc, *parts, *w;
  BP_TRY(ws_get(ctx, "prove.coefs", 4 * n * sizeof(fr_t), (void**)&p.coefs));        // iNTT of a | b | c | PI
  BP_TRY(ws_get(ctx, "prove.abc", 3 * pad * sizeof(fr_t), (void**)&abc));            // a_coeff | b_coeff | c_coeff, n + 2 each
  BP_TRY(ws_get(ctx, "prove.z", 2 * pad * sizeof(fr_t), (void**)&zc));               // z (Lagrange -> coefficients) | z_coeff, n + 3
  BP_TRY(ws_get(ctx, "prove.coset_wit", 20 * n * sizeof(fr_t), (void**)&p.ev));      // a | b | c | z | PI evaluations, 4n each
  BP_TRY(ws_get(ctx, "prove.t", (4 * n + 16) * sizeof(fr_t), (void**)&p.t));
  BP_TRY(ws_get(ctx, "prove.t_parts", 3 * pad * sizeof(fr_t), (void**)&parts));      // t_lo | t_mid | t_hi
  BP_TRY(ws_get(ctx, "prove.num", (n + 16) * sizeof(fr_t), (void**)&p.num));
  BP_TRY(ws_get(ctx, "prove.w", 2 * (n + 16) * sizeof(fr_t), (void**)&w));           // W_zeta | W_zeta_omega
  for (int j = 0; j < 3; j++) { p.coefs5[j] = p.abc[j] = abc + j * pad; p.lens5[j] = n + 2; p.t_part[j] = parts + j * pad; }
  p.z_lag = zc, p.coefs5[3] = p.z_coeff = zc + pad, p.lens5[3] = n + 3;
  p.coefs5[4] = p.coefs + 3 * n, p.lens5[4] = n;
  p.w[0] = w, p.w[1] = w + (n + 16);
  return BP_OK;
}

// ---- round 1 (prover.rs:177-277): a, b, c (and PI) to coefficient form, blinded by (b2 + b1 x)(x^n - 1) etc.
static void blind_column(Prove& p, hipStream_t st, int j) {
  hipLaunchKernelGGL(fr_blind, dim3(blocks_of(p.n + 8)), dim3(256), 0, st, p.coefs + (size_t)j * p.n, p.n, p.blind[2 * j + 1], p.blind[2 * j], Fr::zero(), 2u, p.abc[j]);
}
// the witness is resident: one batch of inverse transforms, three blindings; round1 commits
static int round1_resident(Prove& p) {
  bp_ctx* ctx = p.ctx;
  BP_HIP(ctx, hipMemcpyAsync(p.coefs, p.d_wit, 4 * p.n * sizeof(fr_t), hipMemcpyDeviceToDevice, ctx->stream));
  BP_TRY(ntt_run(ctx, p.coefs, p.cir.log_n, 1, p.pi_zero ? 3 : 4, p.n));        // no public inputs: PI's column is zero and so are its coefficients
  for (int j = 0; j < 3; j++) blind_column(p, ctx->stream, j);
  BP_HIP(ctx, hipGetLastError());
  return BP_OK;
}
// Host witness (ctx.hpp, ProveStaged): per column  upload -> (bytes -> Montgomery) -> inverse transform -> blinding  on the side
// context's stream, an event, and the column's commitment on its lane behind the event.  The host blocks in the pageable copy of
// column j + 1 while the GPU commits to column j: 2.2 ms of uploads at 2^20 gates leave 0.8 on the proof's path.
// Fills p.cm[0..2].  After a failure every launched lane is finished, the side stream is waited for and the first error returned.
static int round1_staged(Prove& p) {
  bp_ctx *ctx = p.ctx, *sd;
  const size_t n = p.n;
  BP_TRY(side_ctx_get(ctx, &sd));
  hipStream_t ss = sd->stream;
  hipEvent_t* seam_ev;                                              // [j]: column j staged (side stream); [3] doubles as the order of the two streams
  BP_TRY(ev_get(ctx, "seam", 4, hipEventDisableTiming, &seam_ev));
  fr_t* wit = const_cast<fr_t*>(p.d_wit);                           // the caller's "prove.witness" workspace: filled here
  BP_HIP(ctx, hipEventRecord(seam_ev[3], ctx->stream));             // behind whatever the context's stream still holds
  BP_HIP(ctx, hipStreamWaitEvent(ss, seam_ev[3], 0));
  MsmPending pend[3];
  int launched = 0, rc = BP_OK;
  for (int j = 0; j < 4 && rc == BP_OK; j++) {
    fr_t *w_j = wit + (size_t)j * n, *c_j = p.coefs + (size_t)j * n;
    hipError_t he;
    if (p.staged->cols[j]) {
      he = hipMemcpyAsync(w_j, p.staged->cols[j], n * sizeof(fr_t), hipMemcpyHostToDevice, ss);
      if (he == hipSuccess && p.staged->fmt == BP_FR_BYTES_LE && fr_convert_run(sd, w_j, n, 0) != BP_OK) he = hipErrorUnknown;
      if (he == hipSuccess) he = hipMemcpyAsync(c_j, w_j, n * sizeof(fr_t), hipMemcpyDeviceToDevice, ss);
      if (he == hipSuccess && ntt_run(sd, c_j, p.cir.log_n, 1, 1, n) != BP_OK) he = hipErrorUnknown;
    } else {                                                        // only PI may be absent: a zero column and zero coefficients
      he = hipMemsetAsync(w_j, 0, n * sizeof(fr_t), ss);
      if (he == hipSuccess) he = hipMemsetAsync(c_j, 0, n * sizeof(fr_t), ss);
    }
    if (he == hipSuccess && j < 3) {
      blind_column(p, ss, j);
      he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipEventRecord(seam_ev[j], ss);
    if (he != hipSuccess) rc = fail(ctx, BP_ERR_HIP, "round 1: staging of a witness column", he, __FILE__, __LINE__);
    else if (j < 3 && (rc = commit_lane_launch(ctx, j, p.srs, p.abc[j], n + 2, seam_ev[j], &pend[j])) == BP_OK) launched = j + 1;
  }
  if (rc == BP_OK) {                                                // rounds 2.. read the columns and coefficients on the context's stream
    const hipError_t he = hipStreamWaitEvent(ctx->stream, seam_ev[3], 0);
    if (he != hipSuccess) rc = fail(ctx, BP_ERR_HIP, "round 1: order", he, __FILE__, __LINE__);
  }
  for (int j = 0; j < launched; j++) {                              // every launched lane is waited for, also after a failure
    const int r2 = commit_lane_finish(ctx, j, pend[j], &p.cm[j]);
    if (rc == BP_OK) rc = r2;
  }
  if (rc != BP_OK) (void)stream_wait(ss);
  return rc;
}
static int round1(Prove& p) {
  bp_ctx *ctx = p.ctx, *side;
  BP_TRY(p.staged ? round1_staged(p) : round1_resident(p));
  if (p.path.early) {                            // round 3 by coset, early part: a, b, c, PI to the shares
    BP_HIP(ctx, hipEventRecord(ctx->ev[4], ctx->stream));
    for (const CosetShare& sh : p.cir.split) {
      DeviceGuard guard(sh.work->device);
      BP_TRY(coset_inputs(p, sh, p.pi_zero ? 0x07u : 0x17u, p.pi_zero, nullptr));
    }
  }
  if (!p.staged) BP_TRY(commit_many(ctx, p.srs, p.abc, p.lens5, 3, &p.cm[0]));        // three independent commitments in flight together
  // Round 3's evaluations of a, b, c and PI on the quotient coset (prover.rs:386-450) depend on no challenge: they are enqueued on the
  // side context's stream once round 1's commitments are in (beside them they only took the GPU from three concurrent pipelines:
  // +2.6 ms on round 1 for -1.9 on round 3) and run beside round 2 -- one commitment, whose sort and tree leave most of the chip idle,
  // and the host's transcript steps.  Round 3 waits for the second event and transforms z alone.  (When: prover_host.hpp, prove_paths.)
  if (p.path.side) {
    BP_TRY(side_ctx_get(ctx, &side));
    BP_TRY(ev_get(ctx, "side", 2, hipEventDisableTiming, &p.side_ev));
    BP_HIP(ctx, hipEventRecord(p.side_ev[0], ctx->stream));
    BP_HIP(ctx, hipStreamWaitEvent(side->stream, p.side_ev[0], 0));
    BP_TRY(lift(ctx, side, coset_eval(side, p.cir, p.coefs5, p.lens5, p.pi_zero ? 0x07u : 0x17u, p.pi_zero, p.ev)));
    BP_HIP(ctx, hipEventRecord(p.side_ev[1], side->stream));
  }
  host_compress48_many(p.proof, &p.cm[0], 3);    // compressed once, into the proof; the transcript absorbs the same 48 bytes (transcript.rs:66-69)
  p.tr.point48("a_1", p.proof); p.tr.point48("b_1", p.proof + 48); p.tr.point48("c_1", p.proof + 96);
  p.beta = p.tr.challenge("beta"), p.gamma = p.tr.challenge("gamma");
  return BP_OK;
}

// ---- round 2 (prover.rs:279-368): permutation grand product, blinded by (b9 + b8 x + b7 x^2)(x^n - 1)
static int round2(Prove& p) {
  bp_ctx* ctx = p.ctx;
  const size_t n = p.n;
  const fr_t *w = p.d_wit, *lag = p.cir.lag;
  BP_TRY(grand_product_run(ctx, w, w + n, w + 2 * n, lag + 5 * n, lag + 6 * n, lag + 7 * n, n, p.beta, p.gamma, fr_from_u64(2), fr_from_u64(3), p.omega,
                           p.z_lag, p.cir.roots));                                   // k1 = 2, k2 = 3 (prover.rs:99-100)
  BP_TRY(ntt_run(ctx, p.z_lag, p.cir.log_n, 1, 1, n));
  hipLaunchKernelGGL(fr_blind, dim3(blocks_of(n + 8)), dim3(256), 0, ctx->stream, p.z_lag, n, p.blind[8], p.blind[7], p.blind[6], 3u, p.z_coeff);
  BP_HIP(ctx, hipGetLastError());
  BP_TRY(commit_many(ctx, p.srs, &p.coefs5[3], &p.lens5[3], 1, &p.cm[3]));           // z_coeff, n + 3
  host_compress48_many(p.proof + 144, &p.cm[3], 1);
  p.tr.point48("z_1", p.proof + 144);
  p.alpha = p.tr.challenge("z_1");                                                   // transcript.rs:24
  return BP_OK;
}

// ---- round 3 (prover.rs:370-500): quotient on the coset g <w_4n>
// p.t = the 4n quotient coefficients, all on this device
static int round3_whole_coset(Prove& p) {
  bp_ctx* ctx = p.ctx;
  const uint32_t k = p.cir.log_n;
  const size_t N = 4 * p.n;
  if (p.path.side) {
    BP_TRY(coset_eval(ctx, p.cir, p.coefs5, p.lens5, 0x08u, false, p.ev));           // z alone ...
    BP_HIP(ctx, hipStreamWaitEvent(ctx->stream, p.side_ev[1], 0));                // ... a, b, c, PI: transformed beside rounds 1-2
  } else {
    BP_TRY(coset_eval(ctx, p.cir, p.coefs5, p.lens5, p.pi_zero ? 0x0Fu : 0x1Fu, p.pi_zero, p.ev));
  }
  hipLaunchKernelGGL(quotient_coset, dim3(blocks_of(N)), dim3(256), 0, ctx->stream, p.ev, p.cir.coset, p.cir.coset_x, N,
                     quotient_args(p.alpha, p.beta, p.gamma, p.cir.cc.zh_inv), p.t, 4u);
  BP_HIP(ctx, hipGetLastError());
  BP_TRY(ntt_run(ctx, p.t, k + 2, 1, 1, N));
  return fr_binary_run(ctx, p.t, N, p.cir.ginv_pow, N, p.t, N, 2);
}
static int round3(Prove& p) {
  bp_ctx* ctx = p.ctx;
  hipStream_t st = ctx->stream;
  const size_t n = p.n;
  BP_TRY(p.path.split ? round3_by_coset(p) : round3_whole_coset(p));
  size_t t_len;
  BP_TRY(fr_nonzero_stats_run(ctx, p.t, 4 * n, 0, 0, &t_len, nullptr));
  // deg(numerator) <= 4n + 5, so an exact quotient has at most 3n + 6 coefficients; anything longer means the division by
  // x^n - 1 left a remainder, i.e. the witness does not satisfy the circuit (the reference would panic at prover.rs:615)
  if (t_len > 3 * n + 6) return BP_FAIL(ctx, BP_ERR_ASSERT, "round 3: constraints not divisible by x^n - 1 (witness does not satisfy the circuit)");
  BP_TRY(fr_squeeze_zeros_run(ctx, p.t, &t_len));
  if (t_len <= 2 * n) return BP_FAIL(ctx, BP_ERR_ASSERT, "round 3: quotient shorter than 2n + 1 (t_hi would be empty; values[0] panics)");
  // split_t_to_3pieces (:649-659) and the blinding of :475-481
  fr_t *t_lo = p.t_part[0], *t_mid = p.t_part[1], *t_hi = p.t_part[2];
  p.hi_len = t_len - 2 * n;
  BP_HIP(ctx, hipMemcpyAsync(t_lo, p.t, n * sizeof(fr_t), hipMemcpyDeviceToDevice, st));
  BP_HIP(ctx, hipMemcpyAsync(t_mid, p.t + n, n * sizeof(fr_t), hipMemcpyDeviceToDevice, st));
  BP_HIP(ctx, hipMemcpyAsync(t_hi, p.t + 2 * n, p.hi_len * sizeof(fr_t), hipMemcpyDeviceToDevice, st));
  BP_HIP(ctx, hipMemcpyAsync(t_lo + n, &p.blind[9], sizeof(fr_t), hipMemcpyHostToDevice, st));      // + b10 x^n
  BP_HIP(ctx, hipMemcpyAsync(t_mid + n, &p.blind[10], sizeof(fr_t), hipMemcpyHostToDevice, st));    // + b11 x^n ...
  hipLaunchKernelGGL(fr_poke_add, dim3(1), dim3(1), 0, st, t_mid, fneg(p.blind[9]));                // ... - b10
  hipLaunchKernelGGL(fr_poke_add, dim3(1), dim3(1), 0, st, t_hi, fneg(p.blind[10]));                // - b11
  BP_HIP(ctx, hipGetLastError());
  const size_t lens[3] = {n + 1, n + 1, p.hi_len};
  BP_TRY(commit_many(ctx, p.srs, p.t_part, lens, 3, &p.cm[4]));
  host_compress48_many(p.proof + 192, &p.cm[4], 3);
  p.tr.point48("t_lo_1", p.proof + 192); p.tr.point48("t_mid_1", p.proof + 240); p.tr.point48("t_hi_1", p.proof + 288);
  p.zeta = p.tr.challenge("zeta");
  return BP_OK;
}

// ---- round 4 (prover.rs:502-541): evaluations at zeta (z at zeta w)
static int round4(Prove& p) {
  const size_t n = p.n;
  // the six evaluations (and PI(zeta), which round 5 wants) in one enqueue and one wait
  const fr_t* polys[7] = {p.abc[0], p.abc[1], p.abc[2], p.cir.coef + 5 * n, p.cir.coef + 6 * n, p.z_coeff, p.coefs + 3 * n};
  const size_t lens[7] = {n + 2, n + 2, n + 2, n, n, n + 3, n};
  const fr_t zw = fmul(p.zeta, p.omega);                                             // z_omega(zeta) = z(zeta w), :661-674
  const fr_t at[7] = {p.zeta, p.zeta, p.zeta, p.zeta, p.zeta, zw, p.zeta};
  fr_t vals[7];
  BP_TRY(poly_eval_many_run(p.ctx, 7, polys, lens, at, vals));
  static const char* const label[6] = {"a_eval", "b_eval", "c_eval", "s1_eval", "s2_eval", "z_shifted_eval"};
  for (int j = 0; j < 6; j++) p.tr.scalar(label[j], p.bar[j] = vals[j]);
  p.pi_zeta = vals[6], p.nu = p.tr.challenge("nu");
  return BP_OK;
}

// ---- round 5 (prover.rs:543-647): linearisation r and the two opening quotients
static int round5(Prove& p) {
  bp_ctx* ctx = p.ctx;
  const size_t n = p.n;
  const fr_t* q = p.cir.coef;                                                        // ql qr qm qo qc s1 s2 s3
  // the opening numerator: the terms in round5_scalars' order (prover_host.hpp)
  const fr_t* const polys[15] = {q + 2 * n, q, q + n, q + 3 * n, q + 4 * n, p.z_coeff, q + 7 * n, p.t_part[0], p.t_part[1], p.t_part[2],
                                 p.abc[0], p.abc[1], p.abc[2], q + 5 * n, q + 6 * n};
  const size_t lens[15] = {n, n, n, n, n, n + 3, n, n + 1, n + 1, p.hi_len, n + 2, n + 2, n + 2, n, n};
  const Round5Scalars sc = round5_scalars(n, p.alpha, p.beta, p.gamma, p.zeta, p.nu, p.bar[0], p.bar[1], p.bar[2], p.bar[3], p.bar[4], p.bar[5], p.pi_zeta);
  LinComb lc;
  memset(&lc, 0, sizeof lc);
  for (int j = 0; j < 15; j++) { lc.p[j] = polys[j]; lc.len[j] = lens[j]; lc.c[j] = sc.c[j]; }
  lc.terms = 15, lc.constant = sc.constant;
  const size_t num_len = std::max(n + 3, p.hi_len);
  if (num_len > n + 16) return BP_FAIL(ctx, BP_ERR_ASSERT, "round 5: quotient piece longer than n + 16");
  hipLaunchKernelGGL(fr_lincomb, dim3(blocks_of(num_len)), dim3(256), 0, ctx->stream, lc, p.num, num_len);
  BP_HIP(ctx, hipGetLastError());
  // r(zeta) == 0 (prover.rs:615): the opening terms vanish at zeta, so the numerator's value there is r's
  fr_t check;
  BP_TRY(poly_eval_run(ctx, p.num, num_len, p.zeta, &check));
  if (!big_is_zero(check)) return BP_FAIL(ctx, BP_ERR_ASSERT, "round 5: r(zeta) != 0 (prover.rs:615)");
  size_t w_len[2];
  BP_TRY(divide_by_linear(ctx, p.num, num_len, p.zeta, p.w[0], &w_len[0]));
  // W_zeta_omega = (z - z_omega_bar) / (x - zeta w)  (:636-638)
  BP_HIP(ctx, hipMemcpyAsync(p.num, p.z_coeff, (n + 3) * sizeof(fr_t), hipMemcpyDeviceToDevice, ctx->stream));
  hipLaunchKernelGGL(fr_poke_add, dim3(1), dim3(1), 0, ctx->stream, p.num, fneg(p.bar[5]));
  BP_HIP(ctx, hipGetLastError());
  BP_TRY(divide_by_linear(ctx, p.num, n + 3, fmul(p.zeta, p.omega), p.w[1], &w_len[1]));
  return commit_many(ctx, p.srs, p.w, w_len, 2, &p.cm[7]);
}

// d_wit: a | b | c | PI Lagrange columns (4 x n, Montgomery, device).  blinders: b1..b11 (prover.rs:110).
int prove_run(bp_ctx* ctx, uint64_t srs, const CircuitEntry& cir, const fr_t* d_wit, const fr_t blind[11], uint8_t proof[624], bool pi_zero,
              const ProveStaged* staged) {
  const fr_t omega = omega_of(cir.log_n);
  if (ctx->side) BP_HIP(ctx, stream_wait(ctx->side->stream));     // side work of a proof that was abandoned half way must not outlive its buffers
  for (const CosetShare& sh : cir.split) {
    DeviceGuard guard(sh.work->device);
    BP_HIP(ctx, stream_wait(sh.work->stream));
  }
  double t[6] = {now_ms()};
  Prove p = {ctx, srs, cir, d_wit, blind, proof, pi_zero, staged, prove_paths_of(ctx, cir, staged != nullptr), (size_t)1 << cir.log_n, omega};
  BP_TRY(prove_workspaces(p));
  int (*const rounds[5])(Prove&) = {round1, round2, round3, round4, round5};
  for (int r = 0; r < 5; r++) {
    BP_TRY(rounds[r](p));
    t[r + 1] = now_ms();
  }
  // ---- Proof (verifier.rs:23-40 field order): 9 compressed points, then the 6 evaluations as 32-byte little-endian
  host_compress48_many(proof + 336, &p.cm[7], 2);                 // the first seven were compressed when the transcript absorbed them
  for (int j = 0; j < 6; j++) fr_to_bytes(proof + 432 + 32 * j, p.bar[j], BP_FR_BYTES_LE);
  for (int r = 0; r < 5; r++) ctx->prove_ms[r] = (float)(t[r + 1] - t[r]);
  ctx->prove_ms[5] = (float)(now_ms() - t[0]);
  return BP_OK;
}

}  // namespace bp

// devcheck.hip -- TEST-ONLY batched wrappers around the product's __host__ __device__ arithmetic headers
// (baby_plonk_rust_amd/csrc/{bigint,fields,fp28,g1,g1_28,fr29,g1_check,msm_digits}.hpp), one case per GPU thread.
//
// Two builds of this one file (tests/devcheck/Makefile):
//   libdevcheck.so       -O3 --offload-arch=gfx950, the product's flags: every dc_<name>(out, in, n) copies the cases to the
//                        card, runs ONE launch of n threads (thread i evaluates case i) and copies the answers back.
//   libdevcheck_host.so  --offload-host-only -DDC_HOST -DBP_HOST_USE_DEVICE_ALGO: the same per-case bodies in a plain loop.
// Every entry point has the same shape: `in` holds n cases of IW 32-bit words, `out` receives n answers of OW words; the
// return value is the HIP status (0 = ok; the host build returns 0).  The per-case body is written once, as a
// __host__ __device__ function both builds call.  Lazy-limb operands (F28<LB, VB>, fr29) cross as raw limbs and are copied
// into the exact type the kernels instantiate, without normalisation: the caller is responsible for the type's bounds.
// Never linked into the product library; includes the product headers by relative path and copies none of their code.
#ifdef DC_HOST
#define BP_HOST_USE_DEVICE_ALGO 1
#endif
#include "../../baby_plonk_rust_amd/csrc/g1_check.hpp"
#include "../../baby_plonk_rust_amd/csrc/g1_28.hpp"
#include "../../baby_plonk_rust_amd/csrc/fr29.hpp"
#include "../../baby_plonk_rust_amd/csrc/msm_digits.hpp"
using namespace bp;

#define DC_HD __host__ __device__ inline
constexpr int DC_MAX_CASES = 1 << 16;
constexpr int DC_BAD_COUNT = 100001;          // n outside [0, 2^16]: nothing is launched

// ---- moving words in and out of the product's types ------------------------------------------------------------------------
template <class T>
DC_HD T ldw(const uint32_t* w) {               // T is a struct of 32-bit limbs only
  T r;
  uint32_t* d = reinterpret_cast<uint32_t*>(&r);
  for (size_t i = 0; i < sizeof(T) / 4; i++) d[i] = w[i];
  return r;
}
template <class T>
DC_HD void stw(uint32_t* w, const T& v) {
  const uint32_t* s = reinterpret_cast<const uint32_t*>(&v);
  for (size_t i = 0; i < sizeof(T) / 4; i++) w[i] = s[i];
}
template <class T>
DC_HD T ld28(const uint32_t* w) {              // 14 raw limbs -> F28<LB, VB>, as they are
  T r;
  for (int i = 0; i < N28; i++) r.l[i] = w[i];
  return r;
}
template <class T>
DC_HD void st28(uint32_t* w, const T& v) {
  for (int i = 0; i < N28; i++) w[i] = v.l[i];
}
DC_HD g1_proj28 ldp28(const uint32_t* w) {     // 42 raw limbs (x | y | z), NOT the padded 44-word memory image
  g1_proj28 r;
  r.x = ld28<C28>(w);
  r.y = ld28<C28>(w + 14);
  r.z = ld28<C28>(w + 28);
  return r;
}
DC_HD void stp28(uint32_t* w, const g1_proj28& p) {
  st28(w, p.x);
  st28(w + 14, p.y);
  st28(w + 28, p.z);
}
DC_HD g1_proj28 to28(const g1_proj& a) {
  g1_proj28 r;
  r.x = widen28<C28>(fp_to_28(a.x));
  r.y = widen28<C28>(fp_to_28(a.y));
  r.z = widen28<C28>(fp_to_28(a.z));
  return r;
}

// ---- the batch driver ------------------------------------------------------------------------------------------------------
#ifndef DC_HOST
template <class Launch>
static int dc_device_run(uint32_t* out, const uint32_t* in, int n, int iw, int ow, Launch launch) {
  if (n < 0 || n > DC_MAX_CASES) return DC_BAD_COUNT;
  if (n == 0) return 0;
  uint32_t *din = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc(&din, (size_t)n * iw * 4);
  if (e == hipSuccess) e = hipMalloc(&dout, (size_t)n * ow * 4);
  if (e == hipSuccess) e = hipMemcpy(din, in, (size_t)n * iw * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0xEE, (size_t)n * ow * 4);         // an answer never written cannot look right
  if (e == hipSuccess) {
    launch(dout, din, n);
    e = hipGetLastError();                                                     // status of the launch ...
  }
  if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * ow * 4, hipMemcpyDeviceToHost);   // ... and of the synchronising copy
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return (int)e;
}
#define DC_ENTRY(name, IW, OW)                                                                     \
  __global__ void __launch_bounds__(64) dck_##name(uint32_t* out, const uint32_t* in, int n) {    \
    const int i = blockIdx.x * blockDim.x + threadIdx.x;                                           \
    if (i >= n) return;                                                                            \
    uint32_t li[IW], lo[OW];                                                                       \
    for (int j = 0; j < IW; j++) li[j] = in[(size_t)i * IW + j];                                   \
    for (int j = 0; j < OW; j++) lo[j] = 0;                                                        \
    body_##name(lo, li);                                                                           \
    for (int j = 0; j < OW; j++) out[(size_t)i * OW + j] = lo[j];                                  \
  }                                                                                                \
  extern "C" int dc_##name(uint32_t* out, const uint32_t* in, int n) {                             \
    return dc_device_run(out, in, n, IW, OW, [](uint32_t* o, const uint32_t* i_, int n_) {         \
      hipLaunchKernelGGL(dck_##name, dim3((n_ + 63) / 64), dim3(64), 0, 0, o, i_, n_);             \
    });                                                                                            \
  }
#else
#define DC_ENTRY(name, IW, OW)                                                   \
  extern "C" int dc_##name(uint32_t* out, const uint32_t* in, int n) {           \
    if (n < 0 || n > DC_MAX_CASES) return DC_BAD_COUNT;                          \
    for (int i = 0; i < n; i++) {                                                \
      uint32_t lo[OW];                                                           \
      for (int j = 0; j < OW; j++) lo[j] = 0;                                    \
      body_##name(lo, in + (size_t)i * IW);                                      \
      for (int j = 0; j < OW; j++) out[(size_t)i * OW + j] = lo[j];              \
    }                                                                            \
    return 0;                                                                    \
  }
#endif

// ---- bigint.hpp / fields.hpp: Fp (12 limbs) and Fr (8 limbs) ---------------------------------------------------------------
#define DC_FIELD(f, F, N)                                                                                                        \
  DC_HD void body_##f##_mul(uint32_t* o, const uint32_t* i) { F::V r; F::mul(r, ldw<F::V>(i), ldw<F::V>(i + N)); stw(o, r); }    \
  DC_ENTRY(f##_mul, 2 * N, N)                                                                                                    \
  DC_HD void body_##f##_sqr(uint32_t* o, const uint32_t* i) { F::V r; F::sqr(r, ldw<F::V>(i)); stw(o, r); }                      \
  DC_ENTRY(f##_sqr, N, N)                                                                                                        \
  DC_HD void body_##f##_add(uint32_t* o, const uint32_t* i) { F::V r; F::add(r, ldw<F::V>(i), ldw<F::V>(i + N)); stw(o, r); }    \
  DC_ENTRY(f##_add, 2 * N, N)                                                                                                    \
  DC_HD void body_##f##_sub(uint32_t* o, const uint32_t* i) { F::V r; F::sub(r, ldw<F::V>(i), ldw<F::V>(i + N)); stw(o, r); }    \
  DC_ENTRY(f##_sub, 2 * N, N)                                                                                                    \
  DC_HD void body_##f##_neg(uint32_t* o, const uint32_t* i) { F::V r; F::neg(r, ldw<F::V>(i)); stw(o, r); }                      \
  DC_ENTRY(f##_neg, N, N)                                                                                                        \
  DC_HD void body_##f##_from_mont(uint32_t* o, const uint32_t* i) { F::V r; F::from_mont(r, ldw<F::V>(i)); stw(o, r); }          \
  DC_ENTRY(f##_from_mont, N, N)                                                                                                  \
  DC_HD void body_##f##_to_mont(uint32_t* o, const uint32_t* i) { F::V r; F::to_mont(r, ldw<F::V>(i)); stw(o, r); }              \
  DC_ENTRY(f##_to_mont, N, N)                                                                                                    \
  DC_HD void body_##f##_pow(uint32_t* o, const uint32_t* i) { F::V r; F::pow(r, ldw<F::V>(i), i + N, N); stw(o, r); }            \
  DC_ENTRY(f##_pow, 2 * N, N)
DC_FIELD(fp, Fp, 12)
DC_FIELD(fr, Fr, 8)
// the inversions: Fermat power in the device build, binary Euclid in the host build (fields.hpp)
DC_HD void body_fp_invert(uint32_t* o, const uint32_t* i) { fp_t r; fp_invert(r, ldw<fp_t>(i)); stw(o, r); }
DC_ENTRY(fp_invert, 12, 12)
DC_HD void body_fr_invert(uint32_t* o, const uint32_t* i) { fr_t r; fr_invert(r, ldw<fr_t>(i)); stw(o, r); }
DC_ENTRY(fr_invert, 8, 8)

// ---- fp28.hpp --------------------------------------------------------------------------------------------------------------
// the operand types of g1_add_mixed28 (g1_28.hpp:80-92), derived from the same expressions so that they follow the header
using MxT0 = decltype(mul28(C28(), F28n()));
using MxT1 = decltype(mul28(C28(), PtY28()));
using MxT3 = decltype(mul28(add28(F28n(), PtY28()), add28(C28(), C28())));
using MxT3s = decltype(norm28(sub28<8, 30>(MxT3(), add28(MxT0(), MxT1()))));
using MxT4 = decltype(add28(mul28(PtY28(), C28()), C28()));
using MxY3a = decltype(norm28(add28(mul28(F28n(), C28()), C28())));
using MxT2 = decltype(norm28(mulk28<12>(C28())));
using MxT1s = decltype(sub28<80, 29>(MxT1(), MxT2()));
using MxY3 = decltype(norm28(mulk28<12>(MxY3a())));
using MxNy3 = decltype(neg28<128, 29>(MxY3()));

DC_HD void body_fp28_roundtrip(uint32_t* o, const uint32_t* i) { stw(o, fp_from_28(fp_to_28(ldw<fp_t>(i)))); }
DC_ENTRY(fp28_roundtrip, 12, 12)
DC_HD void body_fp28_to(uint32_t* o, const uint32_t* i) { st28(o, fp_to_28(ldw<fp_t>(i))); }
DC_ENTRY(fp28_to, 12, 14)
DC_HD void body_fp28_from(uint32_t* o, const uint32_t* i) { stw(o, fp_from_28(ld28<C28>(i))); }               // lazy limbs in
DC_ENTRY(fp28_from, 14, 12)
DC_HD void body_fp28_mul(uint32_t* o, const uint32_t* i) { st28(o, mul28(ld28<C28>(i), ld28<C28>(i + 14))); }
DC_ENTRY(fp28_mul, 28, 14)
DC_HD void body_fp28_mul2(uint32_t* o, const uint32_t* i) {
  st28(o, mul28_2(ld28<C28>(i), ld28<C28>(i + 14), ld28<C28>(i + 28), ld28<C28>(i + 42)));
}
DC_ENTRY(fp28_mul2, 56, 14)
// t3 of the complete addition (g1_28.hpp:105-107): a = X1, b = Y1, c = X2, d = Y2
DC_HD void body_fp28_chain(uint32_t* o, const uint32_t* i) {
  const C28 a = ld28<C28>(i), b = ld28<C28>(i + 14), c = ld28<C28>(i + 28), d = ld28<C28>(i + 42);
  auto t0 = mul28(a, c);
  auto t1 = mul28(b, d);
  st28(o, norm28(sub28<8, 30>(mul28(add28(a, b), add28(c, d)), add28(t0, t1))));
}
DC_ENTRY(fp28_chain, 56, 14)
// x3 of the mixed addition (g1_28.hpp:92) on operands of exactly its types: t3s t1s + t4 (128 p - y3)
DC_HD void body_fp28_neg_mul2(uint32_t* o, const uint32_t* i) {
  st28(o, mul28_2(ld28<MxT3s>(i), ld28<MxT1s>(i + 14), ld28<MxT4>(i + 28), neg28<128, 29>(ld28<MxY3>(i + 42))));
}
DC_ENTRY(fp28_neg_mul2, 56, 14)
// 3b Z1 (g1_28.hpp:86): the raw product by 12, and its one-hop normalisation
DC_HD void body_fp28_mulk12(uint32_t* o, const uint32_t* i) {
  auto m = mulk28<12>(ld28<C28>(i));
  st28(o, m);
  st28(o + 14, norm28(m));
}
DC_ENTRY(fp28_mulk12, 14, 28)
DC_HD void body_fp28_canon(uint32_t* o, const uint32_t* i) { st28(o, canon28(ld28<M28>(i))); }
DC_ENTRY(fp28_canon, 14, 14)
DC_HD void body_fp28_invert(uint32_t* o, const uint32_t* i) { st28(o, fp28_invert(ld28<M28>(i))); }
DC_ENTRY(fp28_invert, 14, 14)
DC_HD void body_fp_invert_via28(uint32_t* o, const uint32_t* i) { fp_t r; fp_invert_via28(r, ldw<fp_t>(i)); stw(o, r); }
DC_ENTRY(fp_invert_via28, 12, 12)

// ---- g1.hpp ----------------------------------------------------------------------------------------------------------------
DC_HD void body_g1_add(uint32_t* o, const uint32_t* i) { g1_proj r; g1_add(r, ldw<g1_proj>(i), ldw<g1_proj>(i + 36)); stw(o, r); }
DC_ENTRY(g1_add, 72, 36)
DC_HD void body_g1_add_mixed(uint32_t* o, const uint32_t* i) { g1_proj r; g1_add_mixed(r, ldw<g1_proj>(i), ldw<g1_affine>(i + 36)); stw(o, r); }
DC_ENTRY(g1_add_mixed, 60, 36)
DC_HD void body_g1_double(uint32_t* o, const uint32_t* i) { g1_proj r; g1_double(r, ldw<g1_proj>(i)); stw(o, r); }
DC_ENTRY(g1_double, 36, 36)
DC_HD void body_g1_mul_scalar(uint32_t* o, const uint32_t* i) { g1_proj r; g1_mul_scalar(r, ldw<g1_proj>(i), ldw<fr_t>(i + 36)); stw(o, r); }
DC_ENTRY(g1_mul_scalar, 44, 36)
DC_HD void body_g1_mul_small(uint32_t* o, const uint32_t* i) { g1_proj r; g1_mul_small(r, ldw<g1_proj>(i), i[36], (int)i[37]); stw(o, r); }
DC_ENTRY(g1_mul_small, 38, 36)
DC_HD void body_g1_to_affine(uint32_t* o, const uint32_t* i) { stw(o, g1_to_affine(ldw<g1_proj>(i))); }
DC_ENTRY(g1_to_affine, 36, 24)

// ---- g1_28.hpp -------------------------------------------------------------------------------------------------------------
// raw forms: one operation on lazy limbs exactly as given, raw limbs out
DC_HD void body_g1_28_add_mixed_raw(uint32_t* o, const uint32_t* i) {            // acc (42) | x2 F28n (14) | y2 PtY28 (14); never the identity point
  g1_proj28 acc = ldp28(i);
  g1_add_mixed28(acc, ld28<F28n>(i + 42), ld28<PtY28>(i + 56));
  stp28(o, acc);
}
DC_ENTRY(g1_28_add_mixed_raw, 70, 42)
DC_HD void body_g1_28_add_raw(uint32_t* o, const uint32_t* i) { g1_proj28 r; g1_add28(r, ldp28(i), ldp28(i + 42)); stp28(o, r); }
DC_ENTRY(g1_28_add_raw, 84, 42)
DC_HD void body_g1_28_double_raw(uint32_t* o, const uint32_t* i) { g1_proj28 r; g1_double28(r, ldp28(i)); stp28(o, r); }
DC_ENTRY(g1_28_double_raw, 42, 42)
DC_HD void body_g1_28_is_identity(uint32_t* o, const uint32_t* i) { o[0] = g1_is_identity28(ldp28(i)) ? 1u : 0u; }
DC_ENTRY(g1_28_is_identity, 42, 1)
// chains from saturated Montgomery operands, as the kernels start from stored points: reps operations, canonical limbs out
DC_HD void body_g1_28_add_mixed(uint32_t* o, const uint32_t* i) {                // acc (36) | affine (24) | neg | reps; the y also comes back
  g1_proj28 acc = to28(ldw<g1_proj>(i));
  const g1_affine28 q = g1_affine_to_28(ldw<g1_affine>(i + 36));
  const PtY28 y = pt_y_signed(q.y, i[60] != 0);
  for (uint32_t k = 0; k < i[61]; k++) g1_add_mixed28(acc, q.x, y);
  stw(o, g1_proj_from_28(acc));
  st28(o + 36, y);
}
DC_ENTRY(g1_28_add_mixed, 62, 50)
DC_HD void body_g1_28_add(uint32_t* o, const uint32_t* i) {                      // a (36) | b (36) | reps: a += b
  g1_proj28 x = to28(ldw<g1_proj>(i));
  const g1_proj28 y = to28(ldw<g1_proj>(i + 36));
  for (uint32_t k = 0; k < i[72]; k++) g1_add28(x, x, y);
  stw(o, g1_proj_from_28(x));
}
DC_ENTRY(g1_28_add, 73, 36)
DC_HD void body_g1_28_double(uint32_t* o, const uint32_t* i) {
  g1_proj28 x = to28(ldw<g1_proj>(i));
  for (uint32_t k = 0; k < i[36]; k++) g1_double28(x, x);
  stw(o, g1_proj_from_28(x));
}
DC_ENTRY(g1_28_double, 37, 36)
DC_HD void body_g1_28_mul_small(uint32_t* o, const uint32_t* i) {
  g1_proj28 r;
  g1_mul_small28(r, to28(ldw<g1_proj>(i)), i[36], (int)i[37]);
  stw(o, g1_proj_from_28(r));
}
DC_ENTRY(g1_28_mul_small, 38, 36)

// The cooperative addition: a (42 raw) | b (42 raw) | reps -> raw limbs.  On the card a case is a group of 8 neighbouring lanes that
// all hold both points, run stage A by role, exchange the six products by shuffles of width 8, run stage B by role and exchange the
// three coordinates -- the split the bucket-reduction kernels use.  The host build walks the roles in a loop.
#ifndef DC_HOST
constexpr int DC_COOP = 8;
__global__ void __launch_bounds__(64) dck_g1_28_add_coop(uint32_t* out, const uint32_t* in, int n) {
  const int lane = blockIdx.x * blockDim.x + threadIdx.x, c = lane / DC_COOP;
  const uint32_t role = threadIdx.x & (DC_COOP - 1);
  const bool live = c < n;                                   // whole groups are live or idle; idle groups still take part in the shuffles
  const int cc = live ? c : 0;
  uint32_t li[85];
  for (int j = 0; j < 85; j++) li[j] = n > 0 ? in[(size_t)cc * 85 + j] : 0;
  g1_proj28 x = ldp28(li);
  const g1_proj28 y = ldp28(li + 42);
  const uint32_t reps = li[84];                              // the same in the 8 lanes of a group: they leave the loop together, and a
                                                             // shuffle of width 8 only reads lanes of its own group
  for (uint32_t k = 0; k < reps; k++) {
    const CoopProd mine = g1_add28_coop_a(role, x, y);
    CoopProd p[6];
    for (int r = 0; r < 6; r++)
      for (int j = 0; j < N28; j++) p[r].l[j] = (uint32_t)__shfl((int)mine.l[j], r, DC_COOP);
    const C28 coord = g1_add28_coop_b(role, p);
    for (int j = 0; j < N28; j++) {
      x.x.l[j] = (uint32_t)__shfl((int)coord.l[j], 0, DC_COOP);
      x.y.l[j] = (uint32_t)__shfl((int)coord.l[j], 1, DC_COOP);
      x.z.l[j] = (uint32_t)__shfl((int)coord.l[j], 2, DC_COOP);
    }
  }
  if (live && role == 0) {
    uint32_t lo[42];
    stp28(lo, x);
    for (int j = 0; j < 42; j++) out[(size_t)c * 42 + j] = lo[j];
  }
}
extern "C" int dc_g1_28_add_coop(uint32_t* out, const uint32_t* in, int n) {
  if (n > DC_MAX_CASES / DC_COOP) return DC_BAD_COUNT;       // at most 2^16 threads per launch
  return dc_device_run(out, in, n, 85, 42, [](uint32_t* o, const uint32_t* i_, int n_) {
    hipLaunchKernelGGL(dck_g1_28_add_coop, dim3((n_ * DC_COOP + 63) / 64), dim3(64), 0, 0, o, i_, n_);
  });
}
#else
DC_HD void body_g1_28_add_coop(uint32_t* o, const uint32_t* i) {
  g1_proj28 x = ldp28(i);
  const g1_proj28 y = ldp28(i + 42);
  for (uint32_t k = 0; k < i[84]; k++) {
    CoopProd prod[6];
    for (uint32_t role = 0; role < 6; role++) prod[role] = g1_add28_coop_a(role, x, y);
    g1_proj28 nx;
    nx.x = g1_add28_coop_b(0, prod);
    nx.y = g1_add28_coop_b(1, prod);
    nx.z = g1_add28_coop_b(2, prod);
    x = nx;
  }
  stp28(o, x);
}
DC_ENTRY(g1_28_add_coop, 85, 42)
#endif

// ---- fr29.hpp: raw 9-limb operands ------------------------------------------------------------------------------------------
DC_HD void body_fr29_from_sat(uint32_t* o, const uint32_t* i) { stw(o, fr29_from_sat(ldw<fr_t>(i))); }
DC_ENTRY(fr29_from_sat, 8, 9)
DC_HD void body_fr29_to_sat_canonical(uint32_t* o, const uint32_t* i) { stw(o, fr29_to_sat_canonical(ldw<fr29>(i))); }
DC_ENTRY(fr29_to_sat_canonical, 9, 8)
DC_HD void body_fr29_mul(uint32_t* o, const uint32_t* i) { stw(o, fr29_mul(ldw<fr29>(i), ldw<fr29>(i + 9))); }
DC_ENTRY(fr29_mul, 18, 9)
DC_HD void body_fr29_add_lazy(uint32_t* o, const uint32_t* i) { stw(o, fr29_add_lazy(ldw<fr29>(i), ldw<fr29>(i + 9))); }
DC_ENTRY(fr29_add_lazy, 18, 9)
DC_HD void body_fr29_sub_lazy(uint32_t* o, const uint32_t* i) { stw(o, fr29_sub_lazy(ldw<fr29>(i), ldw<fr29>(i + 9))); }
DC_ENTRY(fr29_sub_lazy, 18, 9)
DC_HD void body_fr29_butterfly(uint32_t* o, const uint32_t* i) {                 // u | v | w | reps -> u | v
  fr29 u = ldw<fr29>(i), v = ldw<fr29>(i + 9);
  const fr29 w = ldw<fr29>(i + 18);
  for (uint32_t k = 0; k < i[27]; k++) fr29_butterfly(u, v, w);
  stw(o, u);
  stw(o + 9, v);
}
DC_ENTRY(fr29_butterfly, 28, 18)
DC_HD void body_fr29_radix4(uint32_t* o, const uint32_t* i) {                    // a0..a3 | w0..w2 | lazy -> a0..a3
  fr29 a[4], w[3];
  for (int k = 0; k < 4; k++) a[k] = ldw<fr29>(i + 9 * k);
  for (int k = 0; k < 3; k++) w[k] = ldw<fr29>(i + 36 + 9 * k);
  if (i[63]) {
    fr29_radix4(a[0], a[1], a[2], a[3], w[0], w[1], w[2]);
  } else {
    fr29_butterfly(a[0], a[2], w[0]);
    fr29_butterfly(a[1], a[3], w[1]);
    fr29_butterfly(a[0], a[1], w[2]);
    fr29_butterfly(a[2], a[3], w[2]);
  }
  for (int k = 0; k < 4; k++) stw(o + 9 * k, a[k]);
}
DC_ENTRY(fr29_radix4, 64, 36)
DC_HD void body_fr29_reduce8(uint32_t* o, const uint32_t* i) { stw(o, fr29_reduce8(ldw<fr29>(i))); }
DC_ENTRY(fr29_reduce8, 9, 9)
DC_HD void body_fr29_twiddle_from_mont(uint32_t* o, const uint32_t* i) { stw(o, fr29_twiddle_from_mont(ldw<fr_t>(i))); }
DC_ENTRY(fr29_twiddle_from_mont, 8, 9)

// ---- g1_check.hpp ------------------------------------------------------------------------------------------------------------
DC_HD void body_fp_sqrt(uint32_t* o, const uint32_t* i) { fp_t s; o[12] = fp_sqrt(s, ldw<fp_t>(i)) ? 1u : 0u; stw(o, s); }
DC_ENTRY(fp_sqrt, 12, 13)
DC_HD void body_fp_lex_largest(uint32_t* o, const uint32_t* i) { o[0] = fp_lexicographically_largest(ldw<fp_t>(i)) ? 1u : 0u; }
DC_ENTRY(fp_lex_largest, 12, 1)
DC_HD void body_g1_decode48(uint32_t* o, const uint32_t* i) { g1_affine p; o[24] = g1_decode48(p, i); stw(o, p); }
DC_ENTRY(g1_decode48, 12, 25)
DC_HD void body_g1_encode48(uint32_t* o, const uint32_t* i) { g1_encode48(o, ldw<g1_affine>(i)); }
DC_ENTRY(g1_encode48, 24, 12)
DC_HD void body_g1_mul_by_x(uint32_t* o, const uint32_t* i) { g1_proj r; g1_mul_by_x(r, ldw<g1_proj>(i)); stw(o, r); }
DC_ENTRY(g1_mul_by_x, 36, 36)
DC_HD void body_g1_is_torsion_free(uint32_t* o, const uint32_t* i) { o[0] = g1_is_torsion_free(ldw<g1_affine>(i)) ? 1u : 0u; }
DC_ENTRY(g1_is_torsion_free, 24, 1)

// ---- msm_digits.hpp: k (8) | R | m (8) | bias (8) | W -> digit[0..39] | accepted ------------------------------------------------
DC_HD void body_radix_digits(uint32_t* o, const uint32_t* i) {
  const uint32_t W = i[25] > 40 ? 40 : i[25];
  for (int w = 0; w < 40; w++) o[w] = 0x7fffffffu;
  o[40] = msm_radix_digits(i, i[8], i + 9, i + 17, W, [&](uint32_t w, int32_t d) { o[w] = (uint32_t)d; }) ? 1u : 0u;
}
DC_ENTRY(radix_digits, 26, 41)

// ---- what the tables need to know about the header's types (not an entry point: no dc_ prefix) -------------------------------
// out[2k], out[2k+1] = limb bound, value bound of: C28, PtY28, M28, F28n, MxT3s, MxT1s, MxT4, MxY3, MxNy3, CoopSum
extern "C" void devcheck_bounds(uint64_t* out) {
  int k = 0;
#define DC_B(T) out[k++] = T::limb_bound; out[k++] = T::value_bound;
  DC_B(C28) DC_B(PtY28) DC_B(M28) DC_B(F28n) DC_B(MxT3s) DC_B(MxT1s) DC_B(MxT4) DC_B(MxY3) DC_B(MxNy3) DC_B(CoopSum)
#undef DC_B
}

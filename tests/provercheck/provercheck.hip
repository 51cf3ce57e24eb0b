// provercheck.hip -- TEST-ONLY: each kernel of baby_plonk_rust_amd/csrc/prover_kernels.hpp alone, on caller-chosen inputs.
//
// libprovercheck.so (tests/provercheck/Makefile: the product's flags for gfx950) includes the product's header UNCHANGED and has one
// C entry per kernel.  An entry takes host arrays of Montgomery Fr limbs ([k, 4] u64, the memory image of fr_t) and scalars in the
// same form, copies them to the card, launches the product's kernel with the product's launch shape (256 lanes, (count + 255) / 256
// workgroups; fr_blind over n + 8 lanes as prover.hip's blind_column; fr_poke_add <<<1, 1>>>), waits and copies the output back.
// Every OUTPUT buffer is `count + PC_MARGIN` elements long and filled with 0xA5 bytes before the launch (no field element has that
// image: it is above the modulus), body and margin alike; all of it is returned, so the caller sees "wrote zero" apart from "wrote
// nothing" and sees a write behind the end.  The return value is the HIP status (0 = ok) or PC_BAD_ARGS when the arguments would send
// a kernel out of its buffers: then nothing is launched.  tests/test_gpu_prover_kernels.py compares every element with Python integers.
// Never linked into the product library.
#include <vector>

#include "../../baby_plonk_rust_amd/csrc/prover_kernels.hpp"
using namespace bp;

constexpr size_t PC_MARGIN = 8;
constexpr int PC_BAD_ARGS = 100001;
constexpr size_t PC_MAX = (size_t)1 << 20;      // elements per buffer: the tests stay far below

static unsigned blocks_of(size_t threads) { return (unsigned)((threads + 255) / 256); }       // prover.hip
static fr_t fr_of(const uint64_t* limbs) {
  fr_t r;
  memcpy(&r, limbs, sizeof r);
  return r;
}

// device buffers of one entry: freed when the entry returns; after the first failure nothing more is done
struct Run {
  std::vector<void*> owned;
  hipError_t e = hipSuccess;
  fr_t* alloc(size_t count) {
    void* d = nullptr;
    if (e == hipSuccess) e = hipMalloc(&d, (count ? count : 1) * sizeof(fr_t));
    if (d) owned.push_back(d);
    return (fr_t*)d;
  }
  const fr_t* in(const uint64_t* h, size_t count) {
    fr_t* d = alloc(count);
    if (e == hipSuccess && count) e = hipMemcpy(d, h, count * sizeof(fr_t), hipMemcpyHostToDevice);
    return d;
  }
  fr_t* out(size_t count) {
    fr_t* d = alloc(count + PC_MARGIN);
    if (e == hipSuccess) e = hipMemset(d, 0xA5, (count + PC_MARGIN) * sizeof(fr_t));
    return d;
  }
  bool ok() const { return e == hipSuccess; }
  // status of the launch, then the synchronising copy of body and margin
  int back(uint64_t* h, const fr_t* d, size_t count) {
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(h, d, (count + PC_MARGIN) * sizeof(fr_t), hipMemcpyDeviceToHost);
    return (int)e;
  }
  ~Run() {
    for (void* d : owned) (void)hipFree(d);
  }
};

extern "C" {

int pc_margin() { return (int)PC_MARGIN; }

// in, tbl: cap >= len elements each (what lies behind len must not be read into the result); out: n_out + margin
int pc_mul_table_pad(const uint64_t* in, const uint64_t* tbl, size_t cap, size_t len, size_t n_out, uint64_t* out) {
  if (len > cap || cap > PC_MAX || n_out == 0 || n_out > PC_MAX) return PC_BAD_ARGS;
  Run r;
  const fr_t *d_in = r.in(in, cap), *d_tbl = r.in(tbl, cap);
  fr_t* d_out = r.out(n_out);
  if (r.ok()) hipLaunchKernelGGL(fr_mul_table_pad, dim3(blocks_of(n_out)), dim3(256), 0, 0, d_in, len, d_tbl, d_out, n_out);
  return r.back(out, d_out, n_out);
}

// base: n elements; c: c0 c1 c2; out: n + k + margin
int pc_blind(const uint64_t* base, size_t n, const uint64_t* c, uint32_t k, uint64_t* out) {
  if (n == 0 || n > PC_MAX || k > PC_MARGIN) return PC_BAD_ARGS;
  Run r;
  const fr_t* d_base = r.in(base, n);
  fr_t* d_out = r.out(n + k);
  if (r.ok()) hipLaunchKernelGGL(fr_blind, dim3(blocks_of(n + 8)), dim3(256), 0, 0, d_base, n, fr_of(c), fr_of(c + 4), fr_of(c + 8), k, d_out);
  return r.back(out, d_out, n + k);
}

// p: 2 elements, the kernel adds v to the first in place; out: 2 + margin
int pc_poke_add(const uint64_t* p, const uint64_t* v, uint64_t* out) {
  Run r;
  fr_t* d = r.out(2);
  if (r.ok()) r.e = hipMemcpy(d, p, 2 * sizeof(fr_t), hipMemcpyHostToDevice);
  if (r.ok()) hipLaunchKernelGGL(fr_poke_add, dim3(1), dim3(1), 0, 0, d, fr_of(v));
  return r.back(out, d, 2);
}

// polys: terms x cap elements (term k's polynomial starts at k * cap; only len[k] <= cap of them belong to it); coef: terms elements
int pc_lincomb(const uint64_t* polys, size_t cap, const uint64_t* len, const uint64_t* coef, const uint64_t* constant, int terms, size_t n_out,
               uint64_t* out) {
  if (terms < 0 || terms > LINCOMB_MAX || cap > PC_MAX || n_out == 0 || n_out > PC_MAX) return PC_BAD_ARGS;
  for (int k = 0; k < terms; k++)
    if (len[k] > cap) return PC_BAD_ARGS;
  Run r;
  const fr_t* d_polys = r.in(polys, (size_t)terms * cap);
  fr_t* d_out = r.out(n_out);
  LinComb lc;
  memset(&lc, 0, sizeof lc);
  for (int k = 0; k < terms; k++) { lc.p[k] = d_polys + (size_t)k * cap; lc.len[k] = (size_t)len[k]; lc.c[k] = fr_of(coef + 4 * k); }
  lc.terms = terms, lc.constant = fr_of(constant);
  if (r.ok()) hipLaunchKernelGGL(fr_lincomb, dim3(blocks_of(n_out)), dim3(256), 0, 0, lc, d_out, n_out);
  return r.back(out, d_out, n_out);
}

// wit: 5 x N (a b c z PI), pre: 9 x N (ql qr qm qo qc s1 s2 s3 L1), xs: N; QuotientArgs by the product's quotient_args; out: N + margin
int pc_quotient_coset(const uint64_t* wit, const uint64_t* pre, const uint64_t* xs, size_t N, const uint64_t* alpha, const uint64_t* beta,
                      const uint64_t* gamma, const uint64_t* zh_inv, uint32_t zshift, uint64_t* out) {
  if (N == 0 || (N & (N - 1)) || N > PC_MAX) return PC_BAD_ARGS;             // the kernel wraps z(w X) by masking with N - 1
  Run r;
  const fr_t *d_wit = r.in(wit, 5 * N), *d_pre = r.in(pre, 9 * N), *d_xs = r.in(xs, N);
  fr_t* d_out = r.out(N);
  const fr_t zh[4] = {fr_of(zh_inv), fr_of(zh_inv + 4), fr_of(zh_inv + 8), fr_of(zh_inv + 12)};
  if (r.ok())
    hipLaunchKernelGGL(quotient_coset, dim3(blocks_of(N)), dim3(256), 0, 0, d_wit, d_pre, d_xs, N, quotient_args(fr_of(alpha), fr_of(beta), fr_of(gamma), zh),
                       d_out, zshift);
  return r.back(out, d_out, N);
}

// in: cap elements; out[i] = in[i * stride + offset], i < n; out: n + margin
int pc_gather_stride(const uint64_t* in, size_t cap, size_t stride, size_t offset, size_t n, uint64_t* out) {
  if (n == 0 || n > PC_MAX || cap > PC_MAX || stride > 64 || offset > 64 || (n - 1) * stride + offset >= cap) return PC_BAD_ARGS;
  Run r;
  const fr_t* d_in = r.in(in, cap);
  fr_t* d_out = r.out(n);
  if (r.ok()) hipLaunchKernelGGL(fr_gather_stride, dim3(blocks_of(n)), dim3(256), 0, 0, d_in, stride, offset, n, d_out);
  return r.back(out, d_out, n);
}

// c: cap >= len elements; spow: n elements; out: n + margin
int pc_fold_scale(const uint64_t* c, size_t cap, size_t len, size_t n, const uint64_t* s_n, const uint64_t* spow, uint64_t* out) {
  if (n == 0 || n > PC_MAX || len > cap || cap > PC_MAX) return PC_BAD_ARGS;
  Run r;
  const fr_t *d_c = r.in(c, cap), *d_spow = r.in(spow, n);
  fr_t* d_out = r.out(n);
  if (r.ok()) hipLaunchKernelGGL(fr_fold_scale, dim3(blocks_of(n)), dim3(256), 0, 0, d_c, len, n, fr_of(s_n), d_spow, d_out);
  return r.back(out, d_out, n);
}

// v: 4 x n residues; scale: 4 elements; out: 4 n + margin
int pc_coset_recombine(const uint64_t* v, size_t n, const uint64_t* scale, const uint64_t* iinv, uint64_t* out) {
  if (n == 0 || n > PC_MAX / 4) return PC_BAD_ARGS;
  Run r;
  const fr_t* d_v = r.in(v, 4 * n);
  fr_t* d_out = r.out(4 * n);
  const RecombineArgs a = {{fr_of(scale), fr_of(scale + 4), fr_of(scale + 8), fr_of(scale + 12)}, fr_of(iinv)};
  if (r.ok()) hipLaunchKernelGGL(coset_recombine, dim3(blocks_of(n)), dim3(256), 0, 0, d_v, n, a, d_out);
  return r.back(out, d_out, 4 * n);
}

}  // extern "C"

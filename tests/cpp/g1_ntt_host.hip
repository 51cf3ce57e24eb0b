// g1_ntt_host.hip -- TEST-ONLY host build of csrc/g1_ntt.hpp (schedule, butterfly, scalar multiplication and the host loop of the
// inverse transform over G1).  Built by tests/test_g1_ntt_host.py into its tmp_path; never linked into the product library.  With
// -DG1_NTT_MAIN it is a stand-alone program (its own main: one transform of every size up to 16 and a walk over the schedule) for a
// sanitizer run on the CPU (not a pytest test, never run on a GPU):
//   hipcc --offload-host-only -O1 -g -DG1_NTT_MAIN -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/cpp/g1_ntt_host.hip -o g1_ntt_main && ./g1_ntt_main
#include <vector>

#include "../../baby_plonk_rust_amd/csrc/g1_ntt.hpp"
#include "../../baby_plonk_rust_amd/csrc/host_codec.hpp"
using namespace bp;

extern "C" {
// out: i0, i1, e of butterfly b of pass s
void gn_step(uint32_t log_n, uint32_t s, uint64_t b, uint64_t* out) {
  const G1NttStep st = g1_ntt_step(log_n, s, b);
  out[0] = st.i0; out[1] = st.i1; out[2] = st.e;
}
uint64_t gn_bitrev(uint64_t i, uint32_t log_n) { return g1_ntt_bitrev(i, log_n); }
uint32_t gn_max_log() { return G1_NTT_MAX_LOG; }
// out96 = k * p96, k: 32 little-endian bytes, canonical; returns 0, or -1 for a record host_decode96 refuses
int gn_mul(const uint8_t* p96, const uint8_t* k32, uint8_t* out96) {
  g1_proj p;
  fr_t k;
  if (!host_decode96(p, p96)) return -1;
  memcpy(&k, k32, 32);
  g1_ntt_mul(p, p, k);
  host_encode96(out96, p);
  return 0;
}
// 2^log_n points in, 2^log_n points out (96-byte records): g1_ntt_host with the inputs the driver hands the kernel
int gn_transform(const uint8_t* in96, uint32_t log_n, uint8_t* out96) {
  const size_t n = (size_t)1 << log_n;
  std::vector<g1_affine> in(n);
  for (size_t i = 0; i < n; i++) {
    g1_proj p;
    if (!host_decode96(p, in96 + 96 * i)) return -1;
    in[i].x = g1_is_identity(p) ? Fp::zero() : p.x;
    in[i].y = g1_is_identity(p) ? Fp::zero() : p.y;
  }
  std::vector<fr_t> tw(n > 1 ? n / 2 : 1);
  fr_t omega, n_inv;
  (void)host_root_of_unity(omega, (uint64_t)n);
  for (size_t k = 0; k < tw.size(); k++) tw[k] = fr_pow_u64(omega, k);
  fr_invert(n_inv, fr_from_u64((uint64_t)n));
  Fr::from_mont(n_inv, n_inv);
  std::vector<g1_proj> a(n), b(n);
  const g1_proj* r = g1_ntt_host(in.data(), log_n, tw.data(), n_inv, a.data(), b.data());
  for (size_t i = 0; i < n; i++) host_encode96(out96 + 96 * i, r[i]);
  return 0;
}
}

#ifdef G1_NTT_MAIN
#include <stdio.h>
int main() {
  unsigned long sum = 0;
  for (uint32_t log_n = 0; log_n <= 4; log_n++) {
    const size_t n = (size_t)1 << log_n;
    std::vector<uint8_t> in(96 * n), out(96 * n);
    g1_proj p = g1_from_affine(g1_affine_generator());
    for (size_t i = 0; i < n; i++) {
      host_encode96(&in[96 * i], i % 3 == 2 ? g1_identity() : p);
      g1_double(p, p);
    }
    if (gn_transform(in.data(), log_n, out.data())) return 1;
    for (uint8_t v : out) sum += v;
  }
  for (uint32_t log_n = 1; log_n <= G1_NTT_MAX_LOG; log_n++)
    for (uint32_t s = 0; s < log_n; s++) {
      uint64_t o[3];
      gn_step(log_n, s, ((uint64_t)1 << (log_n - 1)) - 1, o);
      if (o[1] >= ((uint64_t)1 << log_n) || o[2] >= ((uint64_t)1 << log_n)) return 2;
      sum += o[0] + gn_bitrev(o[1], log_n);
    }
  printf("g1_ntt_host ok (%lu)\n", sum);
  return 0;
}
#endif

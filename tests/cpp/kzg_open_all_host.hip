// kzg_open_all_host.hip -- TEST-ONLY host build of csrc/kzg_open_all.hpp (the index maps of S^, c^ and the forward-by-reversal rule,
// pass 0 of the three transforms over G1 and the host loop over them, on the butterfly and the multiplication of csrc/g1_ntt.hpp).
// Built by tests/test_kzg_open_all_host.py into its tmp_path; never linked into the product library.  With -DKZG_OPEN_ALL_MAIN it is a
// stand-alone program (its own main: all proofs at n = 2, 4, 8, 16 over points with identities among them, and a walk over the index
// maps up to the largest size) for a sanitizer run on the CPU (not a pytest test, never run on a GPU):
//   hipcc --offload-host-only -O1 -g -DKZG_OPEN_ALL_MAIN -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/cpp/kzg_open_all_host.hip -o kzg_open_all_main && ./kzg_open_all_main
#include <vector>

#include "../../baby_plonk_rust_amd/csrc/kzg_open_all.hpp"
#include "../../baby_plonk_rust_amd/csrc/host_codec.hpp"
using namespace bp;

static std::vector<fr_t> powers(uint64_t len, uint64_t count) {
  fr_t omega;
  (void)host_root_of_unity(omega, len);
  std::vector<fr_t> tw(count ? count : 1);
  for (uint64_t k = 0; k < tw.size(); k++) tw[k] = fr_pow_u64(omega, k);
  return tw;
}

extern "C" {
uint64_t oa_shat(uint32_t log_n, uint64_t j) { return open_all_shat(log_n, j); }
uint64_t oa_chat(uint32_t log_n, uint64_t t) { return open_all_chat(log_n, t); }
uint64_t oa_reversed(uint32_t log_len, uint64_t j) { return open_all_reversed(log_len, j); }
uint64_t oa_forward_source(uint32_t log_len, uint64_t slot) { return open_all_forward_source(log_len, slot); }
uint64_t oa_none() { return OPEN_ALL_NONE; }

// All n = 2^log_n proofs (96-byte records, natural order) of the polynomial with the n_values <= n coefficients coeffs32 (32
// little-endian bytes each, canonical) against the n - 1 points srs96: the table by open_all_table_host, normalised as the driver
// normalises it, the scalars N^-1 DFT_2n(c^) by the definition of the DFT over open_all_chat, the proofs by open_all_proofs_host.
// log_n >= 1.  Returns 0, -1 for a refused point record, -2 for a refused scalar.
int oa_proofs(const uint8_t* srs96, const uint8_t* coeffs32, uint64_t n_values, uint32_t log_n, uint8_t* out96) {
  const uint64_t n = (uint64_t)1 << log_n, N = 2 * n;
  std::vector<g1_affine> srs(n);                           // n - 1 used
  for (uint64_t i = 0; i + 1 < n; i++) {
    g1_proj p;
    if (!host_decode96(p, srs96 + 96 * i)) return -1;
    srs[i].x = g1_is_identity(p) ? Fp::zero() : p.x;
    srs[i].y = g1_is_identity(p) ? Fp::zero() : p.y;
  }
  std::vector<fr_t> f(n, Fr::zero());
  for (uint64_t i = 0; i < n_values; i++)
    if (!fr_from_bytes(f[i], coeffs32 + 32 * i, BP_FR_BYTES_LE)) return -2;
  const std::vector<fr_t> tw_big = powers(N, n), tw_small = powers(n, n / 2), w = powers(N, N);
  std::vector<g1_proj> a(N), b(N);
  const g1_proj* t = open_all_table_host(log_n, srs.data(), tw_big.data(), a.data(), b.data());
  std::vector<g1_affine> table(N);
  for (uint64_t j = 0; j < N; j++) table[j] = g1_to_affine(t[j]);
  fr_t n_inv;
  fr_invert(n_inv, fr_from_u64(N));
  std::vector<fr_t> sc(N);
  for (uint64_t j = 0; j < N; j++) {
    fr_t acc = Fr::zero();
    for (uint64_t k = 0; k < N; k++) {
      const uint64_t src = open_all_chat(log_n, k);
      if (src == OPEN_ALL_NONE) continue;
      fr_t term;
      Fr::mul(term, f[src], w[(j * k) & (N - 1)]);
      Fr::add(acc, acc, term);
    }
    Fr::mul(sc[j], acc, n_inv);
  }
  const g1_proj* r = open_all_proofs_host(log_n, table.data(), sc.data(), tw_big.data(), tw_small.data(), a.data(), b.data());
  for (uint64_t i = 0; i < n; i++) host_encode96(out96 + 96 * i, r[i]);
  return 0;
}
}

#ifdef KZG_OPEN_ALL_MAIN
#include <stdio.h>
int main() {
  unsigned long sum = 0;
  for (uint32_t log_n = 1; log_n <= 4; log_n++) {
    const size_t n = (size_t)1 << log_n;
    std::vector<uint8_t> srs(96 * n), coeffs(32 * n, 0), out(96 * n);
    g1_proj p = g1_from_affine(g1_affine_generator());
    for (size_t i = 0; i + 1 < n; i++) {
      host_encode96(&srs[96 * i], i % 3 == 2 ? g1_identity() : p);
      g1_double(p, p);
    }
    for (size_t i = 0; i < n; i++) coeffs[32 * i] = (uint8_t)(i % 4 == 3 ? 0 : 3 * i + 1), coeffs[32 * i + 9] = (uint8_t)i;
    for (size_t n_values : {n, n - 1, (size_t)1, (size_t)0}) {
      if (oa_proofs(srs.data(), coeffs.data(), n_values, log_n, out.data())) return 1;
      for (uint8_t v : out) sum += v;
    }
  }
  for (uint32_t log_n = 1; log_n < G1_NTT_MAX_LOG; log_n++) {
    const uint64_t n = (uint64_t)1 << log_n, N = 2 * n;
    for (uint64_t j : {(uint64_t)0, (uint64_t)1, n - 2, n - 1, n, N - 1}) {
      const uint64_t s = oa_shat(log_n, oa_forward_source(log_n + 1, j)), c = oa_chat(log_n, j), h = oa_forward_source(log_n, j & (n - 1));
      if ((s != OPEN_ALL_NONE && s + 2 > n) || (c != OPEN_ALL_NONE && c >= n) || h >= n) return 2;
      sum += (s & 0xff) + (c & 0xff) + h;
    }
  }
  printf("kzg_open_all_host ok (%lu)\n", sum);
  return 0;
}
#endif

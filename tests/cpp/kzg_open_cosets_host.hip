// kzg_open_cosets_host.hip -- TEST-ONLY host build of csrc/kzg_open_cosets.hpp (the index maps of S^(j), c^(j) and the cell layout, the
// per-lane bodies of the table, multiplication and halving passes and the host loops over them, on the butterfly and the multiplication
// of csrc/g1_ntt.hpp).  Built by tests/test_kzg_open_cosets_host.py into its tmp_path; never linked into the product library.  With
// -DKZG_OPEN_COSETS_MAIN it is a stand-alone program (its own main: every (log_n, log_l) with log_l < log_n <= 4 over points with
// identities among them, and a walk over the index maps up to the largest size) for a sanitizer run on the CPU (not a pytest test,
// never run on a GPU):
//   hipcc --offload-host-only -O1 -g -DKZG_OPEN_COSETS_MAIN -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/cpp/kzg_open_cosets_host.hip -o kzg_open_cosets_main && ./kzg_open_cosets_main
#include <vector>

#include "../../baby_plonk_rust_amd/csrc/kzg_open_cosets.hpp"
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
uint64_t oc_shat(uint32_t log_n, uint32_t log_l, uint64_t j, uint64_t i) { return open_cosets_shat(log_n, log_l, j, i); }
uint64_t oc_chat(uint32_t log_n, uint32_t log_l, uint64_t j, uint64_t t) { return open_cosets_chat(log_n, log_l, j, t); }
uint64_t oc_value_source(uint32_t log_n, uint32_t log_l, uint64_t c) { return open_cosets_value_source(log_n, log_l, c); }
uint64_t oc_all_shat(uint32_t log_n, uint64_t j) { return open_all_shat(log_n, j); }
uint64_t oc_all_chat(uint32_t log_n, uint64_t t) { return open_all_chat(log_n, t); }
uint64_t oc_none() { return OPEN_ALL_NONE; }

// The r = n / l cell proofs (96-byte records, cell order) of the polynomial with the n_values <= n coefficients coeffs32 (32
// little-endian bytes each, canonical) against the n - l points srs96: the table by open_cosets_table_host, normalised as the driver
// normalises it, the scalars R^-1 DFT_R(c^(j)) by the definition of the DFT over open_cosets_chat, the proofs by
// open_cosets_proofs_host.  log_l < log_n.  Returns 0, -1 for a refused point record, -2 for a refused scalar.
int oc_proofs(const uint8_t* srs96, const uint8_t* coeffs32, uint64_t n_values, uint32_t log_n, uint32_t log_l, uint8_t* out96) {
  const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l, r = n >> log_l, R = 2 * r, used = log_l ? n - l : n - 1;
  std::vector<g1_affine> srs(n);
  for (uint64_t i = 0; i < used; i++) {
    g1_proj p;
    if (!host_decode96(p, srs96 + 96 * i)) return -1;
    srs[i].x = g1_is_identity(p) ? Fp::zero() : p.x;
    srs[i].y = g1_is_identity(p) ? Fp::zero() : p.y;
  }
  std::vector<fr_t> f(n, Fr::zero());
  for (uint64_t i = 0; i < n_values; i++)
    if (!fr_from_bytes(f[i], coeffs32 + 32 * i, BP_FR_BYTES_LE)) return -2;
  const std::vector<fr_t> tw_big = powers(R, r), tw_small = powers(r, r / 2), w = powers(R, R);
  std::vector<g1_proj> a(2 * n), b(2 * n);
  const g1_proj* t = open_cosets_table_host(log_n, log_l, srs.data(), tw_big.data(), a.data(), b.data());
  std::vector<g1_affine> table(2 * n);
  for (uint64_t j = 0; j < 2 * n; j++) table[j] = g1_to_affine(t[j]);
  fr_t R_inv;
  fr_invert(R_inv, fr_from_u64(R));
  std::vector<fr_t> sc(2 * n);
  for (uint64_t j = 0; j < l; j++)
    for (uint64_t i = 0; i < R; i++) {
      fr_t acc = Fr::zero();
      for (uint64_t k = 0; k < R; k++) {
        const uint64_t src = open_cosets_chat(log_n, log_l, j, k);
        if (src == OPEN_ALL_NONE) continue;
        fr_t term;
        Fr::mul(term, f[src], w[(i * k) & (R - 1)]);
        Fr::add(acc, acc, term);
      }
      Fr::mul(sc[j * R + i], acc, R_inv);
    }
  const g1_proj* out = open_cosets_proofs_host(log_n, log_l, table.data(), sc.data(), tw_big.data(), tw_small.data(), a.data(), b.data());
  for (uint64_t i = 0; i < r; i++) host_encode96(out96 + 96 * i, out[i]);
  return 0;
}
}

#ifdef KZG_OPEN_COSETS_MAIN
#include <stdio.h>
int main() {
  unsigned long sum = 0;
  for (uint32_t log_n = 1; log_n <= 4; log_n++)
    for (uint32_t log_l = 0; log_l < log_n; log_l++) {
      const size_t n = (size_t)1 << log_n;
      std::vector<uint8_t> srs(96 * n), coeffs(32 * n, 0), out(96 * n);
      g1_proj p = g1_from_affine(g1_affine_generator());
      for (size_t i = 0; i < n; i++) {
        host_encode96(&srs[96 * i], i % 3 == 2 ? g1_identity() : p);
        g1_double(p, p);
      }
      for (size_t i = 0; i < n; i++) coeffs[32 * i] = (uint8_t)(i % 4 == 3 ? 0 : 3 * i + 1), coeffs[32 * i + 9] = (uint8_t)i;
      for (size_t n_values : {n, n - 1, (size_t)1, (size_t)0}) {
        if (oc_proofs(srs.data(), coeffs.data(), n_values, log_n, log_l, out.data())) return 1;
        for (uint8_t v : out) sum += v;
      }
    }
  for (uint32_t log_n = 1; log_n < G1_NTT_MAX_LOG; log_n++)
    for (uint32_t log_l = 0; log_l < log_n; log_l++) {
      const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l, r = n >> log_l, R = 2 * r;
      for (uint64_t j : {(uint64_t)0, l - 1})
        for (uint64_t i : {(uint64_t)0, (uint64_t)1, r - 2, r - 1, r, R - 1}) {
          const uint64_t s = oc_shat(log_n, log_l, j, i), c = oc_chat(log_n, log_l, j, i), v = oc_value_source(log_n, log_l, (i * l + j) & (n - 1));
          if ((s != OPEN_ALL_NONE && s + l >= n) || (c != OPEN_ALL_NONE && c >= n) || v >= n) return 2;
          sum += (s & 0xff) + (c & 0xff) + v;
        }
    }
  printf("kzg_open_cosets_host ok (%lu)\n", sum);
  return 0;
}
#endif

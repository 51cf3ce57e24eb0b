// kzg_host_host.hip -- TEST-ONLY host build of csrc/kzg_host.hpp (the domain test of an opening point, the barycentric scale, and the
// scalars of bp_kzg_verify_reduce).  Built by tests/test_kzg_host.py into its tmp_path; never linked into the product library.
// Field elements cross as 32 canonical little-endian bytes (BP_FR_BYTES_LE).
#include <vector>

#include "../../baby_plonk_rust_amd/csrc/kzg_host.hpp"
using namespace bp;

static fr_t get(const uint8_t* b32) { fr_t v = Fr::zero(); (void)fr_from_bytes(v, b32, BP_FR_BYTES_LE); return v; }      // the tests pass values < q
static void put(uint8_t* out, const fr_t& v) { fr_to_bytes(out, v, BP_FR_BYTES_LE); }

extern "C" {
// -1: z is off the domain of 2^k points; else m with z = w^m
long long kh_domain_index(const uint8_t* z32, uint32_t k) {
  uint64_t m = 0;
  return kzg_domain_index(get(z32), k, &m) ? (long long)m : -1;
}
void kh_barycentric_scale(const uint8_t* z32, uint32_t k, uint8_t* out32) { put(out32, kzg_barycentric_scale(get(z32), k)); }
// z: m, y: m x count, nu: m or NULL, r: m or NULL;  out: c (m x count) | w (m) | a (m) | g (1)
void kh_reduce_scalars(size_t m, size_t count, const uint8_t* z, const uint8_t* y, const uint8_t* nu, const uint8_t* r, uint8_t* out) {
  std::vector<fr_t> zs(m), ys(m * count), nus(m), rs(m), c(m * count), w(m), a(m);
  for (size_t i = 0; i < m; i++) {
    zs[i] = get(z + 32 * i);
    if (nu) nus[i] = get(nu + 32 * i);
    if (r) rs[i] = get(r + 32 * i);
  }
  for (size_t i = 0; i < m * count; i++) ys[i] = get(y + 32 * i);
  fr_t g;
  kzg_reduce_scalars(m, count, zs.data(), ys.data(), nu ? nus.data() : nullptr, r ? rs.data() : nullptr, c.data(), w.data(), a.data(), &g);
  for (const fr_t& v : c) { put(out, v); out += 32; }
  for (const fr_t& v : w) { put(out, v); out += 32; }
  for (const fr_t& v : a) { put(out, v); out += 32; }
  put(out, g);
}
}

// host_codec_host.hip -- TEST-ONLY host build of csrc/host_codec.hpp (the wire formats and Fr helpers every C ABI entry point goes
// through), with the host's own multiplier as in the product library.  Built by tests/test_host_codec.py into its tmp_path; never
// linked into the product library.  Points cross as memory images: g1_proj = 144 bytes, g1_affine = 96 bytes (Montgomery limbs).
#include "../../baby_plonk_rust_amd/csrc/host_codec.hpp"
using namespace bp;

extern "C" {
int hc_compress_block() { return HOST_COMPRESS_BLOCK; }
int hc_decode96(uint8_t* proj144, const uint8_t* in96) {
  g1_proj p;
  memset(&p, 0xee, sizeof p);                              // a refusal leaves the pattern: the test sees it never reads `out` then
  const bool ok = host_decode96(p, in96);
  memcpy(proj144, &p, 144);
  return ok;
}
void hc_encode96(uint8_t* out96, const uint8_t* proj144) { g1_proj p; memcpy(&p, proj144, 144); host_encode96(out96, p); }
int hc_on_curve(const uint8_t* aff96) { g1_affine a; memcpy(&a, aff96, 96); return g1_affine_on_curve(a); }
void hc_compress48(uint8_t* out48, const uint8_t* proj144) { g1_proj p; memcpy(&p, proj144, 144); host_compress48(out48, p); }
void hc_batch_to_affine(uint8_t* aff96s, const uint8_t* proj144s, int k) {
  host_batch_to_affine(reinterpret_cast<g1_affine*>(aff96s), reinterpret_cast<const g1_proj*>(proj144s), k);
}
void hc_compress48_many(uint8_t* out48s, const uint8_t* proj144s, int k) {
  host_compress48_many(out48s, reinterpret_cast<const g1_proj*>(proj144s), k);
}
int hc_fr_is_canonical(const uint8_t* b32) { return fr_is_canonical(b32); }
int hc_fr_from_bytes(uint8_t* out32, const uint8_t* b32, int fmt) {
  fr_t v;
  memset(&v, 0xee, sizeof v);
  const bool ok = fr_from_bytes(v, b32, fmt);
  memcpy(out32, &v, 32);
  return ok;
}
void hc_fr_to_bytes(uint8_t* b32, const uint8_t* mont32, int fmt) { fr_t v; memcpy(&v, mont32, 32); fr_to_bytes(b32, v, fmt); }
void hc_fr_from_u64(uint8_t* out32, uint64_t v) { const fr_t r = fr_from_u64(v); memcpy(out32, &r, 32); }
void hc_fr_pow_u64(uint8_t* out32, const uint8_t* mont32, uint64_t e) {
  fr_t a;
  memcpy(&a, mont32, 32);
  const fr_t r = fr_pow_u64(a, e);
  memcpy(out32, &r, 32);
}
int hc_root_of_unity(uint8_t* out32, uint64_t order) {
  fr_t w;
  memset(&w, 0xee, sizeof w);
  const bool ok = host_root_of_unity(w, order);
  memcpy(out32, &w, 32);
  return ok;
}
}

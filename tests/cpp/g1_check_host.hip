// g1_check_host.hip -- TEST-ONLY host build of csrc/g1_check.hpp (square root, compressed decode / encode, mul_by_x, subgroup test)
// with the device's 32-bit column multiplier selected, so tests/test_srs_compressed_host.py checks on the CPU the very code the
// SRS kernels run.  Built by that test into its tmp_path; never linked into the product library.
#define BP_HOST_USE_DEVICE_ALGO 1
#include "../../baby_plonk_rust_amd/csrc/g1_check.hpp"
#include <string.h>
using namespace bp;

extern "C" {
// s = sqrt(a) (Montgomery); returns s^2 == a
int gc_fp_sqrt(uint32_t* s, const uint32_t* a) { fp_t x, r; memcpy(&x, a, 48); const bool ok = fp_sqrt(r, x); memcpy(s, &r, 48); return ok; }
// beta as the header has it (canonical limbs)
void gc_fp_beta(uint32_t* out) { for (int i = 0; i < 12; i++) out[i] = fp_beta_canonical(i); }
// 48-byte record -> device affine (x | y Montgomery, identity (0, 0)); returns the reason (0 = accepted)
uint32_t gc_decode48(uint32_t* out96, const uint8_t* rec48) {
  uint32_t w[12];
  memcpy(w, rec48, 48);
  g1_affine p;
  const uint32_t r = g1_decode48(p, w);
  memcpy(out96, &p, 96);
  return r;
}
void gc_encode48(uint8_t* rec48, const uint32_t* in96) {
  g1_affine p;
  memcpy(&p, in96, 96);
  uint32_t w[12];
  g1_encode48(w, p);
  memcpy(rec48, w, 48);
}
void gc_mul_by_x(uint32_t* r, const uint32_t* a) { g1_proj x, z; memcpy(&x, a, 144); g1_mul_by_x(z, x); memcpy(r, &z, 144); }
int gc_is_torsion_free(const uint32_t* in96) { g1_affine p; memcpy(&p, in96, 96); return g1_is_torsion_free(p); }
}

// kzg_recover_host.hip -- TEST-ONLY host build of csrc/kzg_recover.hpp (the plan of a cell recovery, the slices of its root walk, the
// per-lane bodies of the vanishing evaluations, the spread, the division and the check, and the host loop over them with a naive DFT).
// Built by tests/test_kzg_recover_host.py into its tmp_path; never linked into the product library.  With -DKZG_RECOVER_MAIN it is a
// stand-alone program (its own main: every (log_n, log_l) with log_n <= 4 over several presence sets, a corrupted value, and the
// plan's refusals) for a sanitizer run on the CPU (not a pytest test, never run on a GPU):
//   hipcc --offload-host-only -O1 -g -DKZG_RECOVER_MAIN -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/cpp/kzg_recover_host.hip -o kzg_recover_main && ./kzg_recover_main
#include <vector>

#include "../../baby_plonk_rust_amd/csrc/kzg_recover.hpp"
using namespace bp;

extern "C" {
uint32_t rc_walk() { return KZG_RECOVER_WALK; }
uint64_t rc_slices(uint64_t missing) { return recover_slices(missing); }
int rc_shape_ok(uint32_t log_n, uint32_t log_l) { return recover_shape_ok(log_n, log_l); }
// is s^(2^log_n) one?  (it never is: 7 generates Fr*)
int rc_shift_order_divides(uint32_t log_n) { return big_eq(fr_pow_u64(fr_from_u64(KZG_RECOVER_SHIFT), (uint64_t)1 << log_n), Fr::one()); }

// recover_plan; slot and missing have r entries where the shape is supported and are ignored (may be null) otherwise
int rc_plan(const uint32_t* cell_index, uint64_t m, uint32_t log_n, uint32_t log_l, uint64_t d, int32_t* slot, uint32_t* missing, uint64_t* bad,
            uint64_t* n_missing) {
  const RecoverPlan p = recover_plan(cell_index, m, log_n, log_l, d, slot, missing);
  *bad = p.bad;
  *n_missing = p.n_missing;
  return p.err;
}

// Z_dom | Z_cos as 2r canonical little-endian 32-byte values, through recover_vanishing_host (slice by slice over recover_vanishing_partial_at)
void rc_vanishing(uint32_t log_n, uint32_t log_l, const uint32_t* missing, uint64_t n_missing, uint8_t* out32) {
  const uint64_t r = (uint64_t)1 << (log_n - log_l);
  std::vector<fr_t> z(2 * r);
  recover_vanishing_host(log_n, log_l, missing, n_missing, z.data());
  for (uint64_t i = 0; i < 2 * r; i++) fr_to_bytes(out32 + 32 * i, z[i], BP_FR_BYTES_LE);
}

// recover_host with canonical bytes in (m x l values) and out (n coefficients of g, written unless the plan refuses); -100: a value >= q
int rc_recover(uint32_t log_n, uint32_t log_l, const uint32_t* cell_index, const uint8_t* values32, uint64_t m, uint64_t d, uint8_t* out32,
               uint64_t* first_bad) {
  const uint64_t count = log_l < 32 ? m << log_l : 0;
  std::vector<fr_t> v(count ? count : 1);
  for (uint64_t i = 0; i < count; i++)
    if (!fr_from_bytes(v[i], values32 + 32 * i, BP_FR_BYTES_LE)) return -100;
  const bool shape = recover_shape_ok(log_n, log_l);
  std::vector<fr_t> out(shape ? (size_t)1 << log_n : 1);
  const int rc = recover_host(log_n, log_l, cell_index, v.data(), m, d, out.data(), first_bad);
  if (rc == BP_OK || rc == BP_ERR_ASSERT)
    for (uint64_t i = 0; i < out.size(); i++) fr_to_bytes(out32 + 32 * i, out[i], BP_FR_BYTES_LE);
  return rc;
}
}

#ifdef KZG_RECOVER_MAIN
#include <stdio.h>
int main() {
  unsigned long sum = 0;
  for (uint32_t log_n = 0; log_n <= 4; log_n++)
    for (uint32_t log_l = 0; log_l <= log_n; log_l++) {
      const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l, r = n >> log_l;
      for (uint64_t m = 1; m <= r; m += (r > 4 ? 3 : 1)) {
        std::vector<uint32_t> idx(m);
        for (uint64_t i = 0; i < m; i++) idx[i] = (uint32_t)((5 * i + 3) % r);      // r is a power of two: 5 i + 3 is a permutation
        std::vector<uint8_t> values(32 * m * l, 0), out(32 * n);
        for (uint64_t i = 0; i < m * l; i++) values[32 * i] = (uint8_t)(3 * i + 1), values[32 * i + 7] = (uint8_t)i;
        uint64_t bad = 0;
        const int rc = rc_recover(log_n, log_l, idx.data(), values.data(), m, m * l, out.data(), &bad);
        if (rc != BP_OK) return 1;
        if (m * l > 1 && rc_recover(log_n, log_l, idx.data(), values.data(), m, 1, out.data(), &bad) != BP_ERR_ASSERT) return 2;
        for (uint8_t b : out) sum += b;
      }
    }
  const uint32_t twice[3] = {1, 0, 1}, large[1] = {9};
  std::vector<int32_t> slot(4);
  std::vector<uint32_t> missing(4);
  uint64_t bad, count;
  if (rc_plan(twice, 3, 3, 1, 2, slot.data(), missing.data(), &bad, &count) != BP_ERR_INVALID_ARG || bad != 2) return 3;
  if (rc_plan(large, 1, 3, 1, 2, slot.data(), missing.data(), &bad, &count) != BP_ERR_INVALID_ARG || bad != 0) return 4;
  if (rc_plan(twice, 2, 3, 1, 5, slot.data(), missing.data(), &bad, &count) != BP_ERR_LENGTH) return 5;
  if (rc_plan(twice, 2, 30, 1, 2, nullptr, nullptr, &bad, &count) != BP_ERR_TOO_LARGE) return 6;
  printf("kzg_recover_host ok (%lu)\n", sum);
  return 0;
}
#endif

// srs_check_host_host.hip -- the host pieces of the SRS structure checks behind C entries for tests/test_srs_structure_host.py:
// lowest_failing_prefix (csrc/srs_check_host.hpp) over a vector of "this element is bad" flags, and the G2 multiplication behind
// bp_g2_mul / bp_g2_mul_generator (csrc/pairing_host.hpp).  Built with hipcc --offload-host-only: no GPU, no HIP call.
#include <stdint.h>

#include "../../baby_plonk_rust_amd/csrc/pairing_host.hpp"
#include "../../baby_plonk_rust_amd/csrc/srs_check_host.hpp"

extern "C" {
// the prefix [0, k) passes iff none of its elements is flagged; returns lowest_failing_prefix's answer, *calls = its pred calls
uint64_t sc_lowest_failing_prefix(uint64_t n, const uint8_t* bad, uint32_t* calls) {
  auto holds = [&](size_t k) {
    for (size_t i = 0; i < k; i++)
      if (bad[i]) return false;
    return true;
  };
  return (uint64_t)bp::lowest_failing_prefix((size_t)n, holds, calls);
}
uint32_t sc_ceil_log2(uint64_t n) { return bp::ceil_log2((size_t)n); }
int sc_g2_mul(const uint8_t* q192, const uint8_t* k32, uint8_t* out192) { return bp::host_g2_mul(q192, k32, out192); }
int sc_g2_mul_generator(const uint8_t* k32, uint8_t* out192) { return bp::host_g2_mul_generator(k32, out192); }
}

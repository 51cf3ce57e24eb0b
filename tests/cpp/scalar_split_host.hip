// scalar_split_host.hip -- csrc/scalar_split.hpp compiled for the host alone (hipcc --offload-host-only): the lines that cut a scalar into
// its two halves in the kernels of verify_segments_kernels.hpp, callable from tests/test_scalar_split.py.
#include "../../baby_plonk_rust_amd/csrc/scalar_split.hpp"

using namespace bp;

extern "C" {
// n scalars of 8 little-endian 32-bit limbs -> n x (k0 | k1), 4 limbs each
void ss_split(const uint32_t* k, size_t n, uint32_t* out) {
  for (size_t i = 0; i < n; i++) scalar_split_x2(out + 8 * i, out + 8 * i + 4, k + 8 * i);
}
void ss_x2(uint32_t out[4]) {
  for (int i = 0; i < 4; i++) out[i] = bls_x2_limb(i);
}
int ss_bits() { return SCALAR_SPLIT_BITS; }
}

// sigma_decode_host.hip -- TEST-ONLY host build of csrc/sigma_decode.hpp (label -> cell) with the device's 32-bit column multiplier
// selected, so tests/test_sigma_decode_host.py checks on the CPU the very code the sigma_decode kernel runs.  Built by that test
// into its tmp_path; never linked into the product library.
#define BP_HOST_USE_DEVICE_ALGO 1
#include "../../baby_plonk_rust_amd/csrc/sigma_decode.hpp"
#include <string.h>
#include <vector>
using namespace bp;

extern "C" {
// count Montgomery values (32 bytes each) -> the cell each names (3 * row + col) or 0xFFFFFFFF, one sigma_decode_cell per value
void sd_decode_cells(uint32_t log_n, const uint8_t* mont32, size_t count, uint32_t* out) {
  SigmaConsts k;
  SigmaTable tbl;
  sigma_consts(log_n, &k, &tbl);
  for (size_t i = 0; i < count; i++) {
    fr_t s;
    memcpy(&s, mont32 + 32 * i, 32);
    out[i] = sigma_decode_cell(k, tbl.winv, s);
  }
}
// the host loop over three columns of 2^log_n values: target[3 * row + col]; returns the count of values that are no label
size_t sd_decode_columns(uint32_t log_n, const uint8_t* s1, const uint8_t* s2, const uint8_t* s3, uint32_t* target) {
  const size_t n = (size_t)1 << log_n;
  std::vector<fr_t> col[3];
  const uint8_t* src[3] = {s1, s2, s3};
  for (int c = 0; c < 3; c++) {
    col[c].resize(n);
    memcpy(col[c].data(), src[c], 32 * n);
  }
  return sigma_decode_host(log_n, col[0].data(), col[1].data(), col[2].data(), target);
}
// the constants as the header computes them: kn[3] | kinv[3] | winv[24], Montgomery
void sd_consts(uint32_t log_n, uint8_t* out30x32) {
  SigmaConsts k;
  SigmaTable tbl;
  sigma_consts(log_n, &k, &tbl);
  memcpy(out30x32, k.kn, 96);
  memcpy(out30x32 + 96, k.kinv, 96);
  memcpy(out30x32 + 192, tbl.winv, 32 * SIGMA_MAX_LOG_N);
}
}

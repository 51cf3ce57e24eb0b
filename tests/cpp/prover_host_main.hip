// prover_host_main.hip -- stand-alone host program over csrc/prover_host.hpp, through the shim of tests/test_prover_host.py, for a
// sanitizer run on the CPU (not a pytest test, never run on a GPU):
//   hipcc --offload-host-only -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/cpp/prover_host_main.hip -o prover_host_main && ./prover_host_main
// Every buffer is a heap allocation of exactly the size the call may read or write, so a byte too many is a sanitizer report.  The
// values are checked by identities that need no second implementation; the closed forms are tests/test_prover_host.py's.
#include <stdio.h>

#include <vector>

#include "prover_host_host.hip"

static int failures = 0;
#define CHECK(cond)                                          \
  do {                                                       \
    if (!(cond) && failures++ < 20) fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); \
  } while (0)

int main() {
  const fr_t one = Fr::one();
  for (uint32_t log_n : {3u, 10u, 24u}) {
    const uint64_t n = (uint64_t)1 << log_n;
    std::vector<uint8_t> consts(27 * 32), recombine(5 * 32);
    ph_coset_consts(log_n, consts.data(), recombine.data());
    const fr_t w4n = get(&consts[2 * 32]), i4 = get(&consts[4 * 32]), iinv = get(&consts[5 * 32]);
    CHECK(big_eq(fr_pow_u64(w4n, 4 * n), one) && big_eq(fr_pow_u64(w4n, n), i4) && big_eq(fmul(i4, iinv), one));
    for (int j = 0; j < 4; j++) {
      const fr_t s = get(&consts[(7 + j) * 32]), sn = get(&consts[(15 + j) * 32]), zh_inv = get(&consts[(19 + j) * 32]);
      CHECK(big_eq(fr_pow_u64(s, n), sn) && big_eq(fmul(zh_inv, fsub(sn, one)), one));
      CHECK(!memcmp(&recombine[32 * j], &consts[(23 + j) * 32], 32));
    }
    CHECK(!memcmp(&recombine[4 * 32], &consts[5 * 32], 32));
  }
  {
    std::vector<uint8_t> abg(3 * 32), zh(4 * 32), out(11 * 32);
    for (size_t i = 0; i < abg.size(); i++) abg[i] = (uint8_t)(i % 32 == 31 ? 0 : 7 * i + 1);      // top byte 0: below q
    for (size_t i = 0; i < zh.size(); i++) zh[i] = (uint8_t)(i % 32 == 31 ? 0 : 11 * i + 3);
    ph_quotient_args(abg.data(), zh.data(), out.data());
    CHECK(!memcmp(&out[0], &abg[0], 32) && !memcmp(&out[2 * 32], &abg[32], 64) && !memcmp(&out[7 * 32], zh.data(), 128));
    CHECK(big_eq(get(&out[4 * 32]), fadd(get(&abg[32]), get(&abg[32]))) && big_eq(get(&out[6 * 32]), one));
  }
  for (uint64_t n : {(uint64_t)8, (uint64_t)1 << 24}) {
    std::vector<uint8_t> in(12 * 32), out(16 * 32);
    for (size_t i = 0; i < in.size(); i++) in[i] = (uint8_t)(i % 32 == 31 ? 0 : 13 * i + 5);
    ph_round5_scalars(n, in.data(), out.data());
    CHECK(!memcmp(&out[10 * 32], &in[4 * 32], 32) && big_eq(get(&out[4 * 32]), one));               // c[10] = nu, c[4] = 1
    CHECK(big_eq(get(&out[8 * 32]), fmul(get(&out[7 * 32]), fr_pow_u64(get(&in[3 * 32]), n))));      // c[8] = zeta^n c[7]
    memset(in.data(), 0, in.size());
    in[3 * 32] = 1;                                             // zeta = 1: the L1 branch that does not invert
    ph_round5_scalars(n, in.data(), out.data());
    CHECK(big_is_zero(get(&out[7 * 32])));                      // Z = 0
  }
  const std::vector<char> exact = {'1'};                        // one character and no terminator: only the first may be read
  CHECK(ph_knob_tristate(exact.data()) == 1 && ph_knob_tristate(nullptr) == -1 && ph_knob_tristate("") == -1);
  CHECK(ph_prove_paths(18, 1, 0, 0, -1, -1, -1, -1) == (1 | 4) && ph_prove_paths(20, 1, 1, 1, 1, -1, 1, -1) == (2 | 8));
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("prover_host_main ok\n");
  return 0;
}

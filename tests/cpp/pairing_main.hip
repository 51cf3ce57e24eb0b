// pairing_main.hip -- stand-alone host program over csrc/pairing_host.hpp for a sanitizer run on the CPU (not a pytest test, never
// run on a GPU):
//   hipcc --offload-host-only -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/cpp/pairing_main.hip -o pairing_main && ./pairing_main tests/golden
// The generator known answer (pairing(G1, G2) against the Gt::generator() literal of tests/golden/pairing_kats.json, directly and
// through the check of (G1, identity) under x_2 = G2), one bilinearity case and the rejection rules.  Every output
// buffer is a heap allocation of exactly the size the call may write, so a byte too many is a report.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../baby_plonk_rust_amd/csrc/pairing_host.hpp"
using namespace bp;

static int failures = 0;
#define CHECK(cond)                                     \
  do {                                                  \
    if (!(cond)) {                                      \
      failures++;                                       \
      fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); \
    }                                                   \
  } while (0)

static std::vector<uint8_t> le32(uint64_t k) {
  std::vector<uint8_t> v(32, 0);
  for (int i = 0; i < 8; i++) v[i] = (uint8_t)(k >> (8 * i));
  return v;
}

// the twelve Fp of "Gt::generator" in pairing_kats.json: 72 hex strings of 64-bit limbs after the key, little-endian limbs in order
static std::vector<uint8_t> gt_generator_literal(const std::string& path) {
  std::vector<uint8_t> out;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return out;
  std::string text;
  char buf[4096];
  for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, got);
  fclose(f);
  size_t at = text.find("\"Gt::generator\"");
  for (int k = 0; at != std::string::npos && k < 72; k++) {
    at = text.find("\"0x", at + 1);
    if (at == std::string::npos) break;
    const uint64_t limb = strtoull(text.c_str() + at + 1, nullptr, 16);
    for (int i = 0; i < 8; i++) out.push_back((uint8_t)(limb >> (8 * i)));
  }
  return out;
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "tests/golden";
  const std::vector<uint8_t> literal = gt_generator_literal(dir + "/pairing_kats.json");
  if (literal.size() != GT_BYTES) {
    fprintf(stderr, "cannot read the Gt::generator literal in %s\n", dir.c_str());
    return 2;
  }
  // the crate's fixture: record i = i G, 96 bytes
  std::vector<uint8_t> fx(96000);
  FILE* f = fopen((dir + "/g1_uncompressed_valid_test_vectors.dat").c_str(), "rb");
  if (!f || fread(fx.data(), 1, fx.size(), f) != fx.size()) {
    fprintf(stderr, "cannot read the G1 fixture in %s\n", dir.c_str());
    return 2;
  }
  fclose(f);
  auto G1 = [&](int i) { return fx.data() + 96 * i; };

  std::vector<uint8_t> g2(192), x2(192), q6(192), gt_a(GT_BYTES), gt_b(GT_BYTES), gt_c(GT_BYTES);
  CHECK(host_g2_mul_generator(le32(1).data(), g2.data()) == BP_OK);
  CHECK(host_g2_mul_generator(le32(7).data(), x2.data()) == BP_OK);
  CHECK(host_g2_mul_generator(le32(6).data(), q6.data()) == BP_OK);
  // generator: pairing(G1, G2) is also the product of the check of (G1, identity) under x_2 = G2
  CHECK(host_pairing_gt(G1(1), g2.data(), gt_a.data()) == BP_OK);
  CHECK(gt_a == literal);
  {
    std::vector<uint8_t> pair(192, 0), verdict(1), gt(GT_BYTES);
    memcpy(pair.data(), G1(1), 96);
    pair[96] = 0x40;
    size_t bad = 0;
    CHECK(host_pairing_check(g2.data(), pair.data(), 1, 3, verdict.data(), gt.data(), &bad) == BP_OK && bad == SIZE_MAX);
    CHECK(verdict[0] == 0 && gt == literal);
  }
  // bilinearity: e(2 G1, 3 G2) == e(6 G1, G2) == e(G1, 6 G2)
  {
    std::vector<uint8_t> q3(192);
    CHECK(host_g2_mul_generator(le32(3).data(), q3.data()) == BP_OK);
    CHECK(host_pairing_gt(G1(2), q3.data(), gt_a.data()) == BP_OK);
    CHECK(host_pairing_gt(G1(6), g2.data(), gt_b.data()) == BP_OK);
    CHECK(host_pairing_gt(G1(1), q6.data(), gt_c.data()) == BP_OK);
    CHECK(gt_a == gt_b && gt_b == gt_c);
  }
  // verdicts with tau = 7, and the rejections: outputs stay as they were
  {
    const size_t n = 4;
    std::vector<uint8_t> pairs(192 * n, 0), verdicts(n, 0xA5), gt(GT_BYTES * n, 0xA5);
    memcpy(&pairs[0], G1(3), 96);
    memcpy(&pairs[96], G1(21), 96);              // valid
    memcpy(&pairs[192], G1(3), 96);
    memcpy(&pairs[288], G1(22), 96);             // invalid
    pairs[384] = pairs[480] = 0x40;              // (identity, identity)
    pairs[576] = 0x40;
    memcpy(&pairs[672], G1(5), 96);              // (identity, B)
    size_t bad = 0;
    CHECK(host_pairing_check(x2.data(), pairs.data(), n, 1, verdicts.data(), gt.data(), &bad) == BP_OK && bad == SIZE_MAX);
    CHECK(verdicts[0] == 1 && verdicts[1] == 0 && verdicts[2] == 1 && verdicts[3] == 0);
    std::vector<uint8_t> v2(n, 0xA5), g2buf(GT_BYTES * n, 0xA5);
    std::vector<uint8_t> broken = pairs;
    broken[96 * 5 + 95] ^= 1;                    // B of pair 2: identity flag with a coordinate bit
    broken[96 * 3 + 95] ^= 1;                    // B of pair 1: off the curve
    CHECK(host_pairing_check(x2.data(), broken.data(), n, 0, v2.data(), g2buf.data(), &bad) == BP_ERR_BAD_POINT && bad == 1);
    for (uint8_t b : v2) CHECK(b == 0xA5);
    for (uint8_t b : g2buf) CHECK(b == 0xA5);
    std::vector<uint8_t> x2_bad = x2;
    x2_bad[191] ^= 1;
    CHECK(host_pairing_check(x2_bad.data(), pairs.data(), n, 0, v2.data(), g2buf.data(), &bad) == BP_ERR_BAD_POINT && bad == SIZE_MAX);
    std::vector<uint8_t> x2_id(192, 0);
    x2_id[0] = 0x40;
    CHECK(host_pairing_check(x2_id.data(), pairs.data(), n, 0, v2.data(), g2buf.data(), &bad) == BP_ERR_INVALID_ARG);
    CHECK(host_pairing_check(x2.data(), nullptr, 0, 0, nullptr, nullptr, &bad) == BP_OK);
    std::vector<uint8_t> q(32, 0xff);
    CHECK(host_g2_mul_generator(q.data(), x2_bad.data()) == BP_ERR_BAD_SCALAR);
  }
  printf("%s: %d failure(s)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}

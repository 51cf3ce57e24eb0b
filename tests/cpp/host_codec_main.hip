// host_codec_main.hip -- stand-alone host program over csrc/host_codec.hpp for a sanitizer run on the CPU (not a pytest test, never
// run on a GPU):
//   hipcc --offload-host-only -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/cpp/host_codec_main.hip -o host_codec_main && ./host_codec_main tests/golden
// The crate's 1000 uncompressed records go through decode96 / encode96 / compress48; compress48_many runs over consecutive batches of
// every size up to and past its block, each point rescaled by its own z, with the identity first, in the middle, last and in every
// slot.  Every output buffer is a heap allocation of exactly the size the call may write, so a byte too many is a sanitizer report.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../baby_plonk_rust_amd/csrc/host_codec.hpp"
using namespace bp;

static int failures = 0;
#define CHECK(cond, ...)                        \
  do {                                          \
    if (!(cond)) {                              \
      if (failures++ < 20) {                    \
        fprintf(stderr, "FAILED %s: ", #cond);  \
        fprintf(stderr, __VA_ARGS__);           \
        fprintf(stderr, "\n");                  \
      }                                         \
    }                                           \
  } while (0)

static std::vector<uint8_t> slurp(const std::string& path, size_t want) {
  std::vector<uint8_t> v(want);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f || fread(v.data(), 1, want, f) != want || fgetc(f) != EOF) {
    fprintf(stderr, "cannot read %zu bytes from %s\n", want, path.c_str());
    exit(2);
  }
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "tests/golden";
  const std::vector<uint8_t> unc = slurp(dir + "/g1_uncompressed_valid_test_vectors.dat", 96000);
  const std::vector<uint8_t> comp = slurp(dir + "/g1_compressed_valid_test_vectors.dat", 48000);
  uint8_t id48[48] = {0xc0};

  // the fixture round trip; pts[i] = record i under a z of its own (z walks through powers of the generator's x)
  std::vector<g1_proj> pts(1000);
  fp_t z = Fp::one();
  for (int i = 0; i < 1000; i++) {
    g1_proj p;
    CHECK(host_decode96(p, &unc[96 * i]), "record %d", i);
    std::vector<uint8_t> o96(96), o48(48);
    host_encode96(o96.data(), p);
    CHECK(!memcmp(o96.data(), &unc[96 * i], 96), "encode96 of record %d", i);
    host_compress48(o48.data(), p);
    CHECK(!memcmp(o48.data(), &comp[48 * i], 48), "compress48 of record %d", i);
    Fp::mul(z, z, g1_affine_generator().x);
    Fp::mul(pts[i].x, p.x, z);
    Fp::mul(pts[i].y, p.y, z);
    Fp::mul(pts[i].z, p.z, z);
    host_compress48(o48.data(), pts[i]);
    CHECK(!memcmp(o48.data(), &comp[48 * i], 48), "compress48 of record %d rescaled", i);
  }
  CHECK(g1_is_identity(pts[0]), "record 0 is the identity");
  {                                                          // zero coordinates without the infinity flag: decoded, not on the curve
    const std::vector<uint8_t> zeros(96);
    g1_proj p;
    CHECK(host_decode96(p, zeros.data()) && !g1_is_identity(p) && !g1_affine_on_curve(g1_affine{p.x, p.y}), "96 zero bytes");
  }

  // compress48_many: batches of k from record `at` on; holes = slots replaced by the identity (bit j of a mask, or all)
  const int B = HOST_COMPRESS_BLOCK;
  const int sizes[] = {0, 1, 2, 3, 7, 16, B, B + 1, 2 * B, 2 * B + 1};
  int at = 1, batches = 0;
  for (int k : sizes) {
    for (int mode = 0; mode < 6; mode++) {                   // none, first, middle, last, all three, every slot
      if (k == 0 && mode) break;
      std::vector<g1_proj> in(pts.begin() + at, pts.begin() + at + k);     // exactly k points: reading in[k] is a report
      std::vector<uint8_t> want(comp.begin() + 48 * at, comp.begin() + 48 * (at + k)), got(48 * (size_t)k);
      for (int j = 0; j < k; j++) {
        const bool hole = mode == 5 || (mode == 1 && j == 0) || (mode == 2 && j == k / 2) || (mode == 3 && j == k - 1) ||
                          (mode == 4 && (j == 0 || j == k / 2 || j == k - 1));
        if (!hole) continue;
        if (j & 1) in[j] = g1_identity();
        else in[j].z = Fp::zero();                            // (x : y : 0) is the identity too
        memcpy(&want[48 * j], id48, 48);
      }
      host_compress48_many(got.data(), in.data(), k);
      CHECK(got == want, "compress48_many k = %d mode %d from record %d", k, mode, at);
      std::vector<g1_affine> aff(k);
      host_batch_to_affine(aff.data(), in.data(), k);
      for (int j = 0; j < k; j++) {
        uint32_t w[12];
        g1_encode48(w, aff[j]);
        CHECK(!memcmp(w, &want[48 * j], 48) && (g1_affine_is_identity(aff[j]) || g1_affine_on_curve(aff[j])), "batch_to_affine k = %d mode %d slot %d", k, mode, j);
      }
      batches++;
    }
    at += k;
  }

  // the scalar side once, so that the whole header has run under the sanitizer
  uint8_t b32[32], top[32];
  memset(top, 0xff, 32);
  fr_t v, w;
  CHECK(!fr_from_bytes(v, top, BP_FR_BYTES_LE) && !fr_is_canonical(top) && fr_from_bytes(v, top, BP_FR_MONT), "2^256 - 1");
  v = fr_from_u64(~0ull);
  fr_to_bytes(b32, v, BP_FR_BYTES_LE);
  CHECK(fr_from_bytes(w, b32, BP_FR_BYTES_LE) && big_eq(v, w) && b32[7] == 0xff && b32[8] == 0, "u64 round trip");
  CHECK(!host_root_of_unity(w, 0) && host_root_of_unity(w, (uint64_t)1 << 32) && big_eq(w, fr_root_of_unity(false)), "root_of_unity");
  CHECK(host_root_of_unity(w, 2) && big_eq(fr_pow_u64(w, 2), Fr::one()) && !big_eq(w, Fr::one()), "w_2 = -1");

  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("host_codec_main ok: 1000 records, %d compress48_many batches (block %d)\n", batches, B);
  return 0;
}

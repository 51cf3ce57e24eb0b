// test_srs_compressed.cpp -- C++ mirror check of Setup::from_compressed (host/baby_plonk.hpp): the crate's compressed fixture,
// decoded and subgroup-checked on the GPU, commits to the same point as Setup::from_points over its uncompressed twin, and
// powers_of_x_compressed() gives the file back.  argv[1], argv[2]: the compressed and uncompressed fixture files.
#include <cstdio>
#include <fstream>
#include <iterator>

#include "../../baby_plonk_rust_amd/host/baby_plonk.hpp"

using namespace baby_plonk;

template <size_t N>
static std::vector<std::array<uint8_t, N>> read_records(const char* path) {
  std::ifstream f(path, std::ios::binary);
  std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<std::array<uint8_t, N>> out(bytes.size() / N);
  for (size_t i = 0; i < out.size(); i++) std::memcpy(out[i].data(), bytes.data() + N * i, N);
  return out;
}

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "FAILED %s (line %d)\n", #c, __LINE__); \
      return 1;                                                    \
    }                                                              \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const auto comp = read_records<48>(argv[1]);
  const auto unc = read_records<96>(argv[2]);
  CHECK(comp.size() == 1000 && unc.size() == 1000);
  Context& ctx = Context::global();
  std::vector<Scalar> coeffs;
  for (uint64_t i = 0; i < 1000; i++) coeffs.push_back(Scalar::from_u64(i * i * 7919 + 13));
  const Polynomial poly(coeffs, Basis::Monomial);
  for (bool tables : {false, true}) {
    Setup a = Setup::from_compressed(comp, ctx, tables);
    Setup b = Setup::from_points(unc, ctx, tables);
    CHECK(a.commit(poly) == b.commit(poly));
    CHECK(a.powers_of_x() == unc);
    CHECK(a.powers_of_x_compressed() == comp);
    CHECK(b.powers_of_x_compressed() == comp);
  }
  // a rejected record is a Panic that names its index
  auto bad = comp;
  bad[321][0] &= 0x7f;
  bool threw = false;
  try {
    Setup::from_compressed(bad, ctx, false);
  } catch (const Panic& e) {
    threw = e.code == BP_ERR_BAD_POINT && std::string(e.what()).find("point 321 ") != std::string::npos;
  }
  CHECK(threw);
  std::printf("srs compressed ok\n");
  return 0;
}

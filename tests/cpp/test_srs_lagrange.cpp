// test_srs_lagrange.cpp -- C++ mirror check of Setup::lagrange (host/baby_plonk.hpp): over the first 512 points of the crate's
// uncompressed fixture, commit() of a Lagrange polynomial against the Lagrange Setup is commit() of its i_ntt_381 against the powers;
// a one-hot column commits to L_i itself, the all-ones column to P_0 (the Lagrange polynomials sum to 1); the rules are Panics.
// argv[1]: the uncompressed fixture file.
#include <cstdio>
#include <fstream>
#include <iterator>

#include "../../baby_plonk_rust_amd/host/baby_plonk.hpp"

using namespace baby_plonk;

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "FAILED %s (line %d)\n", #c, __LINE__); \
      return 1;                                                    \
    }                                                              \
  } while (0)

template <class F>
static int panic_code(F f) {
  try {
    f();
  } catch (const Panic& e) {
    return e.code;
  }
  return BP_OK;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  const size_t n = 512;
  CHECK(bytes.size() >= 96 * n);
  std::vector<G1> pts(n);
  for (size_t i = 0; i < n; i++) std::memcpy(pts[i].data(), bytes.data() + 96 * i, 96);
  Context& ctx = Context::global();
  std::vector<Scalar> vals, ones(n, Scalar::from_u64(1)), hot(n, Scalar::zero());
  for (uint64_t i = 0; i < n; i++) vals.push_back(Scalar::from_u64(i * i * 7919 + 13));
  hot[137] = Scalar::from_u64(1);
  for (bool tables : {false, true}) {
    Setup powers = Setup::from_points(pts, ctx, tables);
    Setup lag = powers.lagrange(n, tables);
    CHECK(powers.basis() == Basis::Monomial && lag.basis() == Basis::Lagrange);
    const std::vector<G1> l = lag.powers_of_x();
    CHECK(l.size() == n && powers.powers_of_x() == pts);
    CHECK(lag.commit(Polynomial(vals, Basis::Lagrange)) == powers.commit(Polynomial(i_ntt_381(vals, ctx), Basis::Monomial)));
    CHECK(lag.commit(Polynomial(hot, Basis::Lagrange)) == l[137]);
    CHECK(lag.commit(Polynomial(ones, Basis::Lagrange)) == pts[0]);
    CHECK(panic_code([&] { lag.commit(Polynomial(vals, Basis::Monomial)); }) == BP_ERR_BASIS);
    CHECK(panic_code([&] { powers.commit(Polynomial(vals, Basis::Lagrange)); }) == BP_ERR_BASIS);
    CHECK(panic_code([&] { lag.commit(Polynomial(std::vector<Scalar>(vals.begin(), vals.begin() + n / 2), Basis::Lagrange)); }) == BP_ERR_LENGTH);
    CHECK(panic_code([&] { lag.lagrange(4); }) == BP_ERR_BASIS);
    CHECK(panic_code([&] { powers.lagrange(1024); }) == BP_ERR_INVALID_ARG);
    CHECK(panic_code([&] { powers.lagrange(48); }) == BP_ERR_NOT_POW2);
  }
  std::printf("srs lagrange ok\n");
  return 0;
}

// test_srs_structure.cpp -- C++ mirror check of the SRS structure methods of Setup (host/baby_plonk.hpp): check_powers on a clean
// SRS and on one with a replaced point, from_lagrange_points on the exported points of lagrange(), contribute and
// verify_contribution against generate_srs of the product.
#include <cstdio>

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

static std::array<uint8_t, 32> le32(uint64_t lo, uint64_t hi = 0) {
  std::array<uint8_t, 32> b{};
  for (int i = 0; i < 8; i++) {
    b[i] = (uint8_t)(lo >> (8 * i));
    b[8 + i] = (uint8_t)(hi >> (8 * i));
  }
  return b;
}

int main() {
  Context& ctx = Context::global();
  const size_t n = 64;
  const uint64_t tau = 0x1f2e3d4c5b6a7988ull, s = 0x0123456789abcdefull;
  const auto rho = le32(0x9e3779b97f4a7c15ull, 0x8000000000000001ull);        // 128 bits, the top one set
  Setup powers = Setup::generate_srs(n, le32(tau), ctx, false);

  // check_powers: clean, then one replaced point, then the wrong x_2
  CHECK(powers.has_x_2() && powers.check_powers(rho) == Setup::npos);
  std::vector<G1> pts = powers.powers_of_x();
  std::vector<G1> broken = pts;
  broken[37] = pts[5];
  Setup bad = Setup::from_points(broken, ctx, false);
  CHECK(panic_code([&] { bad.check_powers(rho); }) == BP_ERR_INVALID_ARG);     // no x_2 yet
  bad.set_x_2(powers.x_2());
  CHECK(bad.check_powers(rho) == 37);
  bad.set_x_2(g2_mul_generator(le32(tau + 1)));
  CHECK(bad.check_powers(rho) == 1);
  broken = pts;
  broken[0] = pts[1];
  Setup no_gen = Setup::from_points(broken, ctx, false);
  no_gen.set_x_2(powers.x_2());
  CHECK(no_gen.check_powers(rho) == 0 && no_gen.check_powers(rho, false) == 1);

  // adopt: the exported points of lagrange() come back as a Lagrange Setup that commits like it; a swapped pair does not
  Setup lag = powers.lagrange(n, false);
  const std::vector<G1> L = lag.powers_of_x();
  Setup adopted = Setup::from_lagrange_points(L, powers, rho, false);
  CHECK(adopted.basis() == Basis::Lagrange && adopted.powers_of_x() == L && adopted.x_2() == powers.x_2());
  std::vector<Scalar> vals;
  for (uint64_t i = 0; i < n; i++) vals.push_back(Scalar::from_u64(i * i * 7919 + 13));
  CHECK(adopted.commit(Polynomial(vals, Basis::Lagrange)) == lag.commit(Polynomial(vals, Basis::Lagrange)));
  CHECK(adopted.commit(Polynomial(vals, Basis::Lagrange)) == powers.commit(Polynomial(i_ntt_381(vals, ctx), Basis::Monomial)));
  std::vector<G1> swapped = L;
  std::swap(swapped[9], swapped[40]);
  CHECK(panic_code([&] { Setup::from_lagrange_points(swapped, powers, rho, false); }) == BP_ERR_BAD_POINT);
  CHECK(panic_code([&] { Setup::from_lagrange_points(std::vector<G1>(L.begin(), L.begin() + 48), powers, rho, false); }) == BP_ERR_NOT_POW2);
  CHECK(panic_code([&] { Setup::from_lagrange_points(L, lag, rho, false); }) == BP_ERR_BASIS);

  // contribute: the Setup of tau * s, byte for byte, and a contribution that verifies against s G2 only
  Setup next = powers.contribute(le32(s), false);
  const unsigned __int128 prod = (unsigned __int128)tau * s;                    // < 2^128 < q: no reduction
  Setup expected = Setup::generate_srs(n, le32((uint64_t)prod, (uint64_t)(prod >> 64)), ctx, false);
  CHECK(next.powers_of_x() == expected.powers_of_x() && next.x_2() == expected.x_2());
  CHECK(next.x_2() == g2_mul(powers.x_2(), le32(s)));
  CHECK(next.verify_contribution(powers, g2_mul_generator(le32(s)), rho));
  CHECK(!next.verify_contribution(powers, g2_mul_generator(le32(s + 1)), rho));
  CHECK(!next.verify_contribution(expected, g2_mul_generator(le32(s)), rho));
  CHECK(powers.powers_of_x() == pts);
  std::printf("srs structure ok\n");
  return 0;
}

// C++ test of Prover::check_sigma / Prover::check_witness of the host-side mirror (baby_plonk_rust_amd/host/baby_plonk.hpp) on eight
// chained multiplications: row i = (x_i, y_i, x_i y_i), x_(i+1) the product, so sigma ties cell (2, i) to (0, i + 1) and fixes every
// other cell.  Expectations are that closed form.  Needs a GPU; built and run by tests/test_gpu_cpp_witness_check.py.
#include <cstdio>
#include <cstdlib>

#include "../../baby_plonk_rust_amd/host/baby_plonk.hpp"

using namespace baby_plonk;

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) { std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

static Scalar S(uint64_t v) { return Scalar::from_u64(v); }
static Scalar mul(const Scalar& a, const Scalar& b) { return (Polynomial({a}, Basis::Monomial) * b).values[0]; }
static Scalar neg(const Scalar& a) { return (Polynomial({Scalar::zero()}, Basis::Monomial) - Polynomial({a}, Basis::Monomial)).values[0]; }
static std::array<uint8_t, 32> le(uint64_t v) {
  std::array<uint8_t, 32> b{};
  for (int i = 0; i < 8; i++) b[i] = (uint8_t)(v >> (8 * i));
  return b;
}
static bool is(const Cell& c, uint32_t column, uint64_t row) { return c.present && c.column == column && c.row == row; }

int main() {
  const uint64_t n = 8;
  auto roots = roots_of_unity(n);
  auto label = [&](int col, int row) { return mul(S(col + 1), roots[row]); };      // Cell::label, utils.rs:28-37
  auto lag = [&](std::vector<Scalar> v) { return Polynomial(std::move(v), Basis::Lagrange); };
  std::vector<Scalar> a(n), b(n), c(n), s[3] = {std::vector<Scalar>(n), std::vector<Scalar>(n), std::vector<Scalar>(n)};
  uint64_t x = 2;
  for (uint64_t i = 0; i < n; i++) {
    a[i] = S(x), b[i] = S(i + 2), c[i] = S(x * (i + 2));
    x *= i + 2;
    for (int col = 0; col < 3; col++) s[col][i] = label(col, (int)i);              // every cell its own label: the identity ...
  }
  for (uint64_t i = 0; i + 1 < n; i++) {                                           // ... but (2, i) <-> (0, i + 1), program.rs:126-137
    s[2][i] = label(0, (int)i + 1);
    s[0][i + 1] = label(2, (int)i);
  }
  const std::vector<Scalar> zero(n, Scalar::zero());
  auto circuit = [&](const std::vector<Scalar>& s1) {
    return CommonPreprocessedInput{n, lag(zero), lag(zero), lag(std::vector<Scalar>(n, neg(S(1)))), lag(std::vector<Scalar>(n, S(1))), lag(zero),
                                   lag(s1), lag(s[1]), lag(s[2])};
  };
  Setup setup = Setup::generate_srs(n + 6, le(101));
  {
    Prover prover(setup, circuit(s[0]));
    CHECK(prover.check_sigma().ok());
    WitnessReport r = prover.check_witness(a, b, c);
    CHECK(r.ok() && r.first_gate_row == UINT64_MAX && !r.first_copy_cell.present && !r.first_copy_target.present);
    std::vector<Scalar> bad = b;
    bad[3] = S(77);                                                                // b_3 is used once: only row 3's gate fails
    r = prover.check_witness(a, bad, c, zero);
    CHECK(!r.ok() && r.gate_rows == 1 && r.first_gate_row == 3 && r.copy_cells == 0 && !r.first_copy_cell.present);
    bad = c;
    bad[2] = S(77);                                                                // c_2: row 2's gate, and both edges of (2, 2) <-> (0, 3)
    r = prover.check_witness(a, b, bad);
    CHECK(r.gate_rows == 1 && r.first_gate_row == 2 && r.copy_cells == 2 && is(r.first_copy_cell, 2, 2) && is(r.first_copy_target, 0, 3));
    bool refused = false;
    try { prover.check_witness(a, b, std::vector<Scalar>(4)); } catch (const Panic& p) { refused = p.code == BP_ERR_LENGTH; }
    CHECK(refused);
  }
  {
    std::vector<Scalar> s1 = s[0];
    s1[0] = S(4);                                                                  // 4 w^0 is no label; (0, 0) named itself, so it is now nobody's target
    Prover prover(setup, circuit(s1));
    SigmaReport g = prover.check_sigma();
    CHECK(!g.ok() && g.bad_labels == 1 && is(g.first_bad_label, 0, 0) && g.bad_indegree == 1 && is(g.first_bad_indegree, 0, 0));
    bool refused = false;
    try { prover.check_witness(a, b, c); } catch (const Panic& p) { refused = p.code == BP_ERR_INVALID_ARG; }
    CHECK(refused);
  }
  std::printf("witness check mirror ok\n");
  return 0;
}

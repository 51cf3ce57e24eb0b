// poly_rules.hpp -- the reference's rules for the Polynomial operators (polynomial.rs:14-380), the grand product and the roots of unity
// as pure host functions: what it panics on (refused here with a code and the text fail() records) and the sizes that follow from the
// operands' shapes.  The host form and the device form of every operator ask these and nothing else.  No HIP: tests/test_poly_rules.py.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/bp_msm_ntt.h"

namespace bp {

struct PolyRule { int code; const char* what; };       // code == BP_OK: accepted, what == nullptr
constexpr PolyRule RULE_OK = {BP_OK, nullptr};
inline PolyRule rule_monomial(int basis, const char* what) { return basis == BP_BASIS_MONOMIAL ? RULE_OK : PolyRule{BP_ERR_BASIS, what}; }

// Add / Sub<Polynomial>: Lagrange operands of one length (polynomial.rs:85-89, 142-146); Monomial ones are padded to the longer
inline PolyRule rule_addsub(int basis, size_t na, size_t nb, size_t* n) {
  if (basis == BP_BASIS_LAGRANGE && na != nb) return {BP_ERR_LENGTH, "Polynomials must have the same length"};
  *n = na > nb ? na : nb;
  return RULE_OK;
}
// Add / Sub / Mul<Scalar> (op 0 / 1 / 2): nothing to do for an empty input, every value *= s, every value += s (Lagrange Add AND Sub,
// polynomial.rs:126-128), or copy and values[0] += / -= s (Monomial, :62, :123 -- which panics on an empty polynomial)
enum ScalarAction { SCALAR_NOTHING, SCALAR_MUL_ALL, SCALAR_ADD_ALL, SCALAR_FIRST };
inline PolyRule rule_scalar_op(int basis, int op, size_t n, ScalarAction* action) {
  if (op < 0 || op > 2) return {BP_ERR_INVALID_ARG, "op is not 0 (add), 1 (sub) or 2 (mul)"};
  const bool first = op != 2 && basis == BP_BASIS_MONOMIAL;
  if (n == 0 && first) return {BP_ERR_INVALID_ARG, "empty polynomial"};
  *action = n == 0 ? SCALAR_NOTHING : op == 2 ? SCALAR_MUL_ALL : first ? SCALAR_FIRST : SCALAR_ADD_ALL;
  return RULE_OK;
}
// Mul<Polynomial> (polynomial.rs:176-312): target = na + nb - 1 coefficients ([0 ..= n+m], :272), computed at N = 2^k points,
// find_next_power_of_two(n, m) with n = na-1, m = nb-1: the smallest power of two >= n + m + 1 (utils.rs:54-61); transforms end at 2^28
inline PolyRule rule_mul(int basis, size_t na, size_t nb, uint32_t* k, size_t* N, size_t* target) {
  if (basis != BP_BASIS_MONOMIAL) return {BP_ERR_BASIS, "Polynomial * Polynomial: Lagrange basis is todo!() in the reference"};
  if (na == 0 || nb == 0) return {BP_ERR_INVALID_ARG, "empty polynomial (len - 1 underflows, polynomial.rs:248-249)"};
  const size_t cap = (size_t)1 << 28;
  if (na > cap || nb > cap || na + nb - 1 > cap) return {BP_ERR_TOO_LARGE, "product too long"};
  *target = na + nb - 1;
  for (*k = 0; ((size_t)1 << *k) < *target;) ++*k;
  *N = (size_t)1 << *k;
  return RULE_OK;
}
// Div (polynomial.rs:314-380): the basis first, then, on the lengths with trailing zeros trimmed (:325-339): the zero divisor
// panics (:347-348); a dividend shorter than the divisor gives the empty quotient (nq = 0)
inline PolyRule rule_div_basis(int basis) { return rule_monomial(basis, "Div needs the Monomial basis (polynomial.rs:319)"); }
inline PolyRule rule_div(size_t na_eff, size_t nb_eff, size_t* nq) {
  if (nb_eff == 0) return {BP_ERR_DIV_ZERO, "division by the zero polynomial"};
  *nq = na_eff < nb_eff ? 0 : na_eff - nb_eff + 1;
  return RULE_OK;
}
inline PolyRule rule_evaluate(int basis) { return rule_monomial(basis, "coeffs_evaluate needs the Monomial basis"); }       // polynomial.rs:35
inline PolyRule rule_commit(int basis) { return rule_monomial(basis, "commit needs the Monomial basis (setup.rs:34)"); }
// Setup::commit against an SRS that knows its basis: the polynomial's basis must be the SRS's.  A Monomial SRS keeps rule_commit (any
// length: zip truncation, msm.rs:29); a Lagrange SRS (bp_srs_lagrange) takes exactly the srs_len = 2^log_n values it was made for.
inline PolyRule rule_commit_srs(int basis, size_t n, int srs_basis, size_t srs_len) {
  if (srs_basis == BP_BASIS_MONOMIAL) return rule_commit(basis);
  if (basis != BP_BASIS_LAGRANGE) return {BP_ERR_BASIS, "a Lagrange SRS commits to Lagrange polynomials only"};
  return n == srs_len ? RULE_OK : PolyRule{BP_ERR_LENGTH, "a Lagrange SRS commits to polynomials of exactly its length"};
}
inline PolyRule rule_grand_product(size_t n) { return n > ((size_t)1 << 25) ? PolyRule{BP_ERR_TOO_LARGE, "grand product longer than 2^25"} : RULE_OK; }
inline PolyRule rule_roots(uint64_t group_order) {          // roots_of_unity (utils.rs:45-52); 2^32 / 0 panics in root_of_unity (:39-43)
  if (group_order == 0) return {BP_ERR_INVALID_ARG, "group_order == 0"};
  return group_order > ((uint64_t)1 << 28) ? PolyRule{BP_ERR_TOO_LARGE, "group_order > 2^28"} : RULE_OK;
}

}  // namespace bp

// asks a rule from inside a C ABI entry point (ctx.hpp's BP_FAIL): its refusal is recorded on ctx and returned
#define BP_RULE(ctx, rule) do { const ::bp::PolyRule r__ = (rule); if (r__.code != BP_OK) return BP_FAIL(ctx, r__.code, r__.what); } while (0)

// poly_rules_host.hip -- TEST-ONLY host build of csrc/poly_rules.hpp (the reference's rules for the Polynomial operators, the grand
// product and the roots of unity).  Built by tests/test_poly_rules.py into its tmp_path; never linked into the product library.
// Every shim returns the rule's code; outputs the rule leaves alone keep the caller's pattern; *has_text says whether a text came along.
#include "../../baby_plonk_rust_amd/csrc/poly_rules.hpp"
using namespace bp;

static int told(const PolyRule& r, int* has_text) {
  *has_text = r.what != nullptr && r.what[0] != 0;
  return r.code;
}
extern "C" {
int pr_addsub(int basis, size_t na, size_t nb, size_t* n, int* has_text) { return told(rule_addsub(basis, na, nb, n), has_text); }
int pr_scalar_op(int basis, int op, size_t n, int* action, int* has_text) {      // *action is written only where the rule accepted
  ScalarAction a = SCALAR_NOTHING;
  const int rc = told(rule_scalar_op(basis, op, n, &a), has_text);
  if (rc == BP_OK) *action = (int)a;
  return rc;
}
int pr_action(int which) { return which == 0 ? SCALAR_NOTHING : which == 1 ? SCALAR_MUL_ALL : which == 2 ? SCALAR_ADD_ALL : SCALAR_FIRST; }
int pr_mul(int basis, size_t na, size_t nb, uint32_t* k, size_t* N, size_t* target, int* has_text) {
  return told(rule_mul(basis, na, nb, k, N, target), has_text);
}
int pr_div(size_t na_eff, size_t nb_eff, size_t* nq, int* has_text) { return told(rule_div(na_eff, nb_eff, nq), has_text); }
int pr_div_basis(int basis, int* has_text) { return told(rule_div_basis(basis), has_text); }
int pr_evaluate(int basis, int* has_text) { return told(rule_evaluate(basis), has_text); }
int pr_commit(int basis, int* has_text) { return told(rule_commit(basis), has_text); }
int pr_grand_product(size_t n, int* has_text) { return told(rule_grand_product(n), has_text); }
int pr_roots(uint64_t group_order, int* has_text) { return told(rule_roots(group_order), has_text); }
}

// commit_rule_host.hip -- TEST-ONLY host build of rule_commit_srs (csrc/poly_rules.hpp): the commit rule of an SRS that knows its basis.
// Built by tests/test_srs_lagrange_abi.py into its tmp_path; never linked into the product library.
#include "../../baby_plonk_rust_amd/csrc/poly_rules.hpp"
using namespace bp;

// the rule's code; *has_text = whether a refusal carries its text
extern "C" int cr_commit_srs(int basis, size_t n, int srs_basis, size_t srs_len, int* has_text) {
  const PolyRule r = rule_commit_srs(basis, n, srs_basis, srs_len);
  *has_text = r.what != nullptr;
  return r.code;
}

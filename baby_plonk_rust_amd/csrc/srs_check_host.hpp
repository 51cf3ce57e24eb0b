// srs_check_host.hpp -- the search bp_srs_check_powers and bp_srs_adopt_lagrange run when a check fails: which is the lowest element
// that breaks it?  A pure host function with no HIP include and no bp_ctx, so tests/test_srs_structure_host.py runs it on the CPU
// against every position of one and of two breaks.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bp {

// pred(k), 1 <= k <= n: does the check over the first k elements pass?  Monotone: once a prefix holds a bad element every longer
// one fails.  Returns the lowest k whose prefix fails -- element k - 1 is the lowest bad one -- or SIZE_MAX when pred(n) holds (and
// for n == 0, without a call).  The whole range is asked first, so a clean input costs ONE call; a failing one is bisected between
// the longest prefix known to pass (0: the empty one) and the shortest known to fail: at most 1 + ceil(log2 n) calls in all.
// *calls (may be null) receives the number of calls made.
template <class Pred>
inline size_t lowest_failing_prefix(size_t n, Pred&& pred, uint32_t* calls = nullptr) {
  uint32_t made = 0;
  size_t lo = 0, hi = SIZE_MAX;
  if (n != 0) {
    made++;
    if (!pred(n)) {
      hi = n;
      while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        made++;
        if (pred(mid)) lo = mid; else hi = mid;
      }
    }
  }
  if (calls) *calls = made;
  return hi;
}

// ceil(log2 n) for n >= 1 (0 for n <= 1): the bound above, as the tests and the entry points state it
inline uint32_t ceil_log2(size_t n) {
  uint32_t k = 0;
  while (k < 8 * sizeof(size_t) - 1 && ((size_t)1 << k) < n) k++;
  return k;
}

}  // namespace bp

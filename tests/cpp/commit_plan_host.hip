// commit_plan_host.hip -- TEST-ONLY host build of csrc/commit_plan.hpp (shard arithmetic and the route of a commit_many).  Built by
// tests/test_commit_plan.py into its tmp_path; never linked into the product library.  With -DCOMMIT_PLAN_MAIN it is a stand-alone program
// (its own main: the grid of the test, every plan once, the properties checked in C++) for a sanitizer run on the CPU (not a pytest test,
// never run on a GPU):
//   hipcc --offload-host-only -O1 -g -DCOMMIT_PLAN_MAIN -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/cpp/commit_plan_host.hip -o commit_plan_main && ./commit_plan_main
#include "../../baby_plonk_rust_amd/csrc/commit_plan.hpp"
using namespace bp;

extern "C" {
// commit_plan over shards (first[r], n_shard[r], table_c[r]), r < R, under the default MSM knobs.  Returns the number of rounds; the
// first `cap` of them go to rounds as (base, cnt) pairs.
int cp_plan(uint32_t R, const uint64_t* first, const uint64_t* n_shard, const uint32_t* table_c, uint64_t n_global, int k, const uint64_t* lens, int group,
            int knob, int* route, int* width, int* rounds, int cap) {
  std::vector<CommitShard> sh(R);
  for (uint32_t r = 0; r < R; r++) sh[r] = {(size_t)first[r], (size_t)n_shard[r], table_c[r]};
  std::vector<size_t> n(lens, lens + (k > 0 ? k : 0));
  const CommitPlan p = commit_plan(sh.data(), R, (size_t)n_global, k, n.data(), group != 0, knob, MsmKnobs());
  *route = p.route;
  *width = p.width;
  for (size_t i = 0; i < p.rounds.size() && (int)i < cap; i++) rounds[2 * i] = p.rounds[i].base, rounds[2 * i + 1] = p.rounds[i].cnt;
  return (int)p.rounds.size();
}
void cp_shard_range(uint64_t n, uint64_t r, uint64_t R, uint64_t* lo, uint64_t* hi) {
  size_t a, b;
  shard_range((size_t)n, (size_t)r, (size_t)R, &a, &b);
  *lo = a, *hi = b;
}
void cp_shard_cut(uint64_t first, uint64_t n, uint64_t n_global, uint64_t shard_first, uint64_t shard_n, uint64_t* lo, uint64_t* hi) {
  size_t a, b;
  shard_cut((size_t)first, (size_t)n, (size_t)n_global, (size_t)shard_first, (size_t)shard_n, &a, &b);
  *lo = a, *hi = b;
}
uint64_t cp_shard_slice(uint64_t n_j, uint64_t n_global, uint64_t shard_first, uint64_t shard_n) {
  return shard_slice((size_t)n_j, (size_t)n_global, (size_t)shard_first, (size_t)shard_n);
}
// the widths of the four routes, in the order of CommitRoute
void cp_widths(int out[4]) {
  out[COMMIT_GROUP_BATCH] = out[COMMIT_DEVICE_BATCH] = (int)MSM_MAX_BATCH;
  out[COMMIT_SHARDED] = MSM_SLOTS;
  out[COMMIT_LANES] = MAX_LANES;
}
}

#ifdef COMMIT_PLAN_MAIN
#include <stdio.h>
// the grid of tests/test_commit_plan.py: members, SRS lengths, counts, lengths at every seam, tables on all / none / all but one shard, three
// widths, the knob unset / 0 / 1.  Checked here: the rounds cover 0 .. k once, in order, none wider than its route's limit; the slices of every
// vector over the shards are ascending, disjoint and together [0, min(n_j, n_global)); a range cut over the shards likewise.
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); return 1; } \
  } while (0)
int main() {
  int widths[4];
  cp_widths(widths);
  uint64_t seed = 0x2545F4914F6CDD1Dull;
  auto rnd = [&seed](uint64_t m) { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (seed >> 33) % m; };
  unsigned long plans = 0, by_route[4] = {0, 0, 0, 0};
  for (uint32_t R = 1; R <= 8; R++)
    for (uint64_t n_global : {1ull, 7ull, 8ull, 1000ull, 1001ull, (1ull << 20) + 6})
      for (int k = 0; k <= 9; k++)
        for (int tables = 0; tables < 3; tables++)
          for (uint32_t c : {6u, 16u, 20u})
            for (int knob = -1; knob <= 1; knob++) {
              uint64_t first[8], len[8], pick[32], lens[9];
              uint32_t tc[8], n_pick = 0;
              const uint32_t missing = (uint32_t)rnd(R);
              for (uint32_t r = 0; r < R; r++) {
                uint64_t lo, hi;
                cp_shard_range(n_global, r, R, &lo, &hi);
                CHECK(lo <= hi && hi <= n_global && (r == 0 ? lo == 0 : lo == first[r - 1] + len[r - 1]) && (r + 1 < R || hi == n_global));
                first[r] = lo, len[r] = hi - lo;
                tc[r] = tables == 0 || (tables == 2 && r == missing) ? 0 : c;
                if (r) pick[n_pick++] = lo ? lo - 1 : 0, pick[n_pick++] = lo, pick[n_pick++] = lo + 1;
              }
              for (uint64_t v : {0ull, 1ull, (unsigned long long)n_global, (unsigned long long)n_global + 9}) pick[n_pick++] = v;
              for (int j = 0; j < k; j++) lens[j] = pick[rnd(n_pick)];
              int route, width, rounds[2 * 9];
              const int n_rounds = cp_plan(R, first, len, tc, n_global, k, lens, R > 1, knob, &route, &width, rounds, 9);
              CHECK(route >= 0 && route < 4 && width == widths[route] && n_rounds <= 9);
              CHECK((R > 1) == (route == COMMIT_GROUP_BATCH || (route == COMMIT_SHARDED && k != 1)) || k <= 1);
              int at = 0;
              for (int i = 0; i < n_rounds; i++) {
                CHECK(rounds[2 * i] == at && rounds[2 * i + 1] >= 1 && rounds[2 * i + 1] <= width);
                at += rounds[2 * i + 1];
              }
              CHECK(at == (k > 0 ? k : 0));
              for (int j = 0; j < k; j++) {
                uint64_t end = 0;
                for (uint32_t r = 0; r < R; r++) {
                  const uint64_t s = cp_shard_slice(lens[j], n_global, first[r], len[r]);
                  CHECK(s <= len[r] && (s == 0 || first[r] == end));
                  end += s;
                }
                CHECK(end == (lens[j] < n_global ? lens[j] : n_global));
                const uint64_t from = pick[rnd(n_pick)];
                uint64_t covered = 0;
                for (uint32_t r = 0; r < R; r++) {
                  uint64_t lo, hi;
                  cp_shard_cut(from, lens[j], n_global, first[r], len[r], &lo, &hi);
                  if (lo >= hi) continue;
                  CHECK(lo >= from && lo >= first[r] && hi <= first[r] + len[r] && (covered == 0 || lo == first[r]));
                  covered += hi - lo;
                }
                CHECK(covered == (from > n_global ? 0 : (lens[j] < n_global - from ? lens[j] : n_global - from)));
              }
              plans++, by_route[route]++;
            }
  // the edge of the batched pipeline (c = 16, J = 4, two members of m points): 2 097 215 points per member fit one pipeline, 2 097 216 do not
  for (uint64_t m : {2097215ull, 2097216ull}) {
    const uint64_t first[2] = {0, m}, len[2] = {m, m}, lens[8] = {1000, 1000, 1000, 1000, 2 * m, 2 * m, 2 * m, 2 * m};
    const uint32_t tc[2] = {16, 16};
    int route, width, rounds[16];
    for (int k : {3, 4})
      CHECK(cp_plan(2, first, len, tc, 2 * m, k, lens + 4, 1, -1, &route, &width, rounds, 8) == 1 &&
            route == (m == 2097216 && k == 4 ? COMMIT_SHARDED : COMMIT_GROUP_BATCH));
    CHECK(cp_plan(2, first, len, tc, 2 * m, 8, lens, 1, -1, &route, &width, rounds, 8) == 2 && route == (m == 2097216 ? COMMIT_SHARDED : COMMIT_GROUP_BATCH));
    plans += 3;
  }
  printf("commit_plan_host ok (%lu plans: %lu group batches, %lu sharded, %lu device batches, %lu lanes)\n", plans, by_route[0], by_route[1], by_route[2], by_route[3]);
  return 0;
}
#endif

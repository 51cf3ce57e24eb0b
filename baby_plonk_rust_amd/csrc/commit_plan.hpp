// commit_plan.hpp -- everything Setup::commit decides from numbers alone: which points of an SRS lie on which shard, which part of a
// scalar vector a shard multiplies, and the route k commitments of one call take (commit_many, capi_msm.hip) with its rounds.
// Host-pure: no HIP runtime call and no bp_ctx; tests/test_commit_plan.py compiles it for the host alone and enumerates it.
#pragma once
#include <stddef.h>

#include <vector>

#include "msm_plan.hpp"

namespace bp {

// ---- shard arithmetic
// contiguous point range [lo, hi) of shard r of R over n points; the first n % R shards get one extra point
inline void shard_range(size_t n, size_t r, size_t R, size_t* lo, size_t* hi) {
  const size_t base = n / R, extra = n % R;
  *lo = r * base + (r < extra ? r : extra);
  *hi = *lo + base + (r < extra ? 1 : 0);
}
// the part [lo, hi) of points [first, first + n) on the shard that holds [shard_first, shard_first + shard_n), in global indices;
// n is cut to the SRS's length first (zip() truncation, msm.rs:29), a range that starts behind the SRS is empty.  lo >= hi: none of it.
inline void shard_cut(size_t first, size_t n, size_t n_global, size_t shard_first, size_t shard_n, size_t* lo, size_t* hi) {
  const size_t room = first > n_global ? 0 : n_global - first, end = first + (n < room ? n : room);
  *lo = first > shard_first ? first : shard_first;
  *hi = end < shard_first + shard_n ? end : shard_first + shard_n;
}
// scalars of a vector of n_j, multiplied against points 0 .. n_j of the SRS, that belong to that shard: they start at element shard_first
inline size_t shard_slice(size_t n_j, size_t n_global, size_t shard_first, size_t shard_n) {
  const size_t nj = n_j < n_global ? n_j : n_global;              // zip() truncation, msm.rs:29
  return nj > shard_first ? (nj - shard_first < shard_n ? nj - shard_first : shard_n) : 0;
}

// ---- the route of one commit_many
struct CommitShard {
  size_t first, n;       // global index of its first point, points on it
  uint32_t table_c;      // width of its fixed-base tables; 0: none
};
enum CommitRoute : int {
  COMMIT_GROUP_BATCH,    // group: ONE pipeline per member over its slices of up to MSM_MAX_BATCH commitments (msm_launch_many)
  COMMIT_SHARDED,        // every shard queues its part of up to MSM_SLOTS commitments back to back, one pipeline each
  COMMIT_DEVICE_BATCH,   // one device: ONE pipeline over up to MSM_MAX_BATCH commitments
  COMMIT_LANES,          // one device: up to MAX_LANES commitments at a time, each on a lane (context, stream and workspaces of its own)
};
constexpr int MAX_LANES = 3;
enum : int { COMMIT_KNOB_UNSET = -1 };      // BP_COMMIT_BATCH as the plan takes it: unset (and any value that is neither), 0, 1
struct CommitRound {
  int base, cnt;         // commitments [base, base + cnt) of the call
};
struct CommitPlan {
  CommitRoute route;
  int width;             // most commitments a round of this route takes
  std::vector<CommitRound> rounds;
};

// the slices of vectors n[0 .. cnt) on a shard -> lens; returns their sum (0: the shard takes no part in this round)
inline size_t commit_slices(const CommitShard& s, size_t n_global, const size_t* n, int cnt, size_t* lens) {
  size_t total = 0;
  for (int j = 0; j < cnt; j++) total += lens[j] = shard_slice(n[j], n_global, s.first, s.n);
  return total;
}
// does every round of MSM_MAX_BATCH commitments fit ONE pipeline on every shard that takes part in it?  Asked of msm_plan before
// anything is enqueued, so a call that does not fit goes one by one from its first commitment on and no batch runs in vain.
inline bool commit_batches_fit(const CommitShard* sh, size_t R, size_t n_global, int k, const size_t* n, const MsmKnobs& kn) {
  for (int base = 0; base < k; base += (int)MSM_MAX_BATCH) {
    const int cnt = k - base < (int)MSM_MAX_BATCH ? k - base : (int)MSM_MAX_BATCH;
    for (size_t r = 0; r < R; r++) {
      size_t lens[MSM_MAX_BATCH];
      if (commit_slices(sh[r], n_global, n + base, cnt, lens) == 0) continue;
      if (msm_plan((uint32_t)cnt, lens, sh[r].table_c, sh[r].n, false, kn).err == BP_ERR_TOO_LARGE) return false;
    }
  }
  return true;
}

// The route of k >= 1 commitments of vectors of n[j] scalars against an SRS of n_global points held by sh[0 .. R) (a plain context:
// its one entry), and the rounds it runs in.
//   A batch -- one sort keyed (polynomial, bucket), one accumulation, one fix-up, one tree over J x 2^(c-1) buckets -- pays the
//   latency-bound tail once per round instead of once per commitment.  It needs fixed-base tables on every shard and rounds short
//   enough for the partition sort (commit_batches_fit).
//   The members of a group, whose shards are short and whose pipelines share one stream each, batch by default (BP_COMMIT_BATCH=0
//   turns it off); the tables are used whatever the slice lengths: skipping them for very short slices is a speed heuristic of
//   the single path.  Without tables, with one commitment or with a round that does not fit: queued shards.
//   On ONE device the concurrent lanes already hide the tails of two commitments under the accumulation of the third, and the
//   batch's three-fold sort is exposed: measured 35.6 ms per 2^20-gate proof against 34.4-35.4 with lanes
//   (profiles/r03_commit_batch_ab.txt), so the batch runs only on request there (BP_COMMIT_BATCH=1) and where the tables pay for the
//   longest vector; a single commitment takes the sharded route over its one shard.
inline CommitPlan commit_plan(const CommitShard* sh, size_t R, size_t n_global, int k, const size_t* n, bool group, int knob, const MsmKnobs& kn) {
  bool batch = k > 1 && (group ? knob != 0 : knob == 1);
  for (size_t r = 0; r < R && batch; r++) batch = sh[r].table_c != 0;
  if (batch && !group) {
    size_t n_max = 0;
    for (int j = 0; j < k; j++) {
      const size_t len = shard_slice(n[j], n_global, sh[0].first, sh[0].n);
      if (len > n_max) n_max = len;
    }
    batch = srs_width_pays(sh[0].table_c, n_max);
  }
  batch = batch && commit_batches_fit(sh, R, n_global, k, n, kn);
  CommitPlan p;
  if (batch) p.route = group ? COMMIT_GROUP_BATCH : COMMIT_DEVICE_BATCH, p.width = (int)MSM_MAX_BATCH;
  else if (group || k == 1) p.route = COMMIT_SHARDED, p.width = MSM_SLOTS;      // one pinned result slot per commitment in flight on a stream
  else p.route = COMMIT_LANES, p.width = MAX_LANES;
  for (int base = 0; base < k; base += p.width) p.rounds.push_back({base, k - base < p.width ? k - base : p.width});
  return p;
}

}  // namespace bp

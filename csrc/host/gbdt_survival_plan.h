// survival:cox bookkeeping: the scans' tiles, the workspace of a plan and the
// tie runs of the sorted times. Free of torch and HIP (csrc/tests/
// gbdt_survival_plan_test.cc runs it without a GPU).
//
// A plan holds the rows in the stable ascending order of t = |y|. Rows with
// equal t form a tie run and share one risk set. Position i knows its run's
// first and last position (head, tail) and, at the head only, the run's
// number of events (run_events; 0 elsewhere). With S_i the inclusive suffix
// sum of e at position i, the run's D is S at its head, so
//   r_i = sum over heads k <= i of run_events_k / S_k,
//   q_i = sum over heads k <= i of run_events_k / S_k^2
// are inclusive prefix sums at position i itself: every row of a run sees all
// of the run's events, and neither scan looks up a value of another tile.
#pragma once

#include <cstdint>

namespace wh {

// the scans' tile: kCoxThreads threads x kCoxItems consecutive positions
constexpr int kCoxThreads = 256;
constexpr int kCoxItems = 8;
constexpr int kCoxTile = kCoxThreads * kCoxItems;

inline int64_t gbdt_cox_tile() { return kCoxTile; }
inline int64_t gbdt_cox_tiles(int64_t n) { return n <= 0 ? 0 : (n + kCoxTile - 1) / kCoxTile; }

// The plan's fp64 workspace, in doubles: {m*}, the sorted e [n], the suffix
// sums S [n], the tiles' partials (4 per tile: the stats' need) and the tiles'
// exclusive offsets (1 per tile of the suffix scan, then 2 per tile: the
// forward scan's two channels).
struct CoxWs {
  int64_t mstar, e, S, part, off, off2, size;
};
inline CoxWs gbdt_cox_ws(int64_t n) {
  const int64_t nt = gbdt_cox_tiles(n);
  CoxWs w;
  w.mstar = 0;
  w.e = 1;
  w.S = w.e + n;
  w.part = w.S + n;
  w.off = w.part + 4 * nt;
  w.off2 = w.off + nt;
  w.size = w.off2 + 2 * nt;
  return w;
}

// The tie runs of ascending times t [n], delta [n] (1: event): head / tail
// [n] = the first / last position of the position's run, run_events [n] =
// the run's events at its head, 0 elsewhere. Returns the number of events.
// (Position a opens its run whatever t[a] is, so a NaN time -- equal to
// nothing, itself included -- is a run of one and the loop always advances.)
inline int64_t gbdt_cox_runs(const float* t, const uint8_t* delta, int64_t n, int32_t* head,
                             int32_t* tail, int32_t* run_events) {
  int64_t total = 0;
  for (int64_t a = 0; a < n;) {
    int64_t b = a + 1;
    int32_t ev = delta[a] ? 1 : 0;
    while (b < n && t[b] == t[a]) ev += delta[b++] ? 1 : 0;
    for (int64_t i = a; i < b; ++i) {
      head[i] = (int32_t)a;
      tail[i] = (int32_t)(b - 1);
      run_events[i] = 0;
    }
    run_events[a] = ev;
    total += ev;
    a = b;
  }
  return total;
}

}  // namespace wh

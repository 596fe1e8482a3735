// The rule that gives a GBDT node its weight and its children their
// constraints, said once for every grower: the host grower
// (csrc/bind/gbdt_ops.cc gbdt_grow), the device level loop and the best-first
// leaf loop (gbdt.hip gd_apply / leaf_pick) and the bounded split search
// evaluate these functions, so they give a node the same bits and pick the
// same splits. Only arithmetic in which no fused multiply-add can form lives
// here; the gains stay in gbdt.hip under their fp-contract pragma. Free of
// torch; HIP only for the function qualifiers. The Python mirrors are
// models/gbdt.py child_bounds and models/gbdt_objective.py interaction_child.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define WH_NODE_FN __host__ __device__ __forceinline__
#else
#define WH_NODE_FN inline
#endif

namespace wh {

// The L1 threshold T(G) of alpha
WH_NODE_FN double gbdt_l1(double G, double alpha) {
  return alpha <= 0 ? G : (G > alpha ? G - alpha : (G < -alpha ? G + alpha : 0.0));
}

// The unclamped node weight -T(G) / (H + lambda), 0 below min_child_weight
WH_NODE_FN double gbdt_weight0(double G, double H, double alpha, double lambda, double mcw) {
  return H >= mcw ? -gbdt_l1(G, alpha) / (H + lambda) : 0.0;
}

// monotone_constraints: a node's weight interval. A weight is clamped to it;
// an accepted split on a feature of sign c cuts it at the mean of the
// children's clamped weights (wl, wr): c > 0 gives the left child {lo, mid}
// and the right {mid, hi}, c < 0 the mirror image, c == 0 hands the interval
// down unchanged. The root's is (-inf, inf), or max_delta_step on either side
// of 0.
struct GbdtBounds {
  double lo, hi;
};

struct GbdtChildBounds {
  GbdtBounds left, right;
};

WH_NODE_FN double gbdt_clamp_weight(double w, const GbdtBounds& b) {
  return w < b.lo ? b.lo : (w > b.hi ? b.hi : w);
}

// (the weight of a node with totals (G, H) inside its interval)
WH_NODE_FN double gbdt_weight(double G, double H, double alpha, double lambda, double mcw,
                              const GbdtBounds& b) {
  return gbdt_clamp_weight(gbdt_weight0(G, H, alpha, lambda, mcw), b);
}

WH_NODE_FN GbdtChildBounds gbdt_child_bounds(int c, const GbdtBounds& b, double wl, double wr) {
  const double mid = (wl + wr) / 2;
  if (c > 0) return {{b.lo, mid}, {mid, b.hi}};
  if (c < 0) return {{mid, b.hi}, {b.lo, mid}};
  return {b, b};
}

// interaction_constraints on one 64-bit word: bit i < 63 of a feature's mask
// says that group i contains it, and a feature in no group holds bit 63 alone.
// A node's state is the set of groups that contain every feature split on
// above it: all ones at the root, which therefore admits every feature; a
// node admits feature f iff state & mask[f] != 0. The children of a split on
// f narrow the state by mask[f] and drop bit 63, so nothing is admitted below
// a split on an ungrouped feature.
constexpr uint64_t kGbdtInterFree = 1ull << 63;
constexpr uint64_t kGbdtInterRoot = ~0ull;

WH_NODE_FN bool gbdt_admits(uint64_t state, uint64_t fmask) { return (state & fmask) != 0; }

WH_NODE_FN uint64_t gbdt_child_state(uint64_t state, uint64_t fmask) {
  return state & fmask & ~kGbdtInterFree;
}

}  // namespace wh

// The exact per-leaf weighted quantile of the adaptive objectives
// (reg:absoluteerror, reg:quantileerror; docs/bsp_apps.md "Absolute and
// quantile error"): an MSD radix select with 8-bit digits, four passes over an
// order-preserving 32-bit key of the residual. Here: the key transform, the
// fixed-point weight, the threshold, the digit pick and the task plan -- what
// the kernels (csrc/hip/gbdt_quantile.hip), the binding and the stand-alone
// self-test (csrc/tests/gbdt_quantile_plan_test.cc) share. Free of torch; HIP
// only for the function qualifiers.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define WH_QSEL_FN __host__ __device__ __forceinline__
#else
#define WH_QSEL_FN inline
#endif

namespace wh {

constexpr int kQselBins = 256;   // one 8-bit digit
constexpr int kQselPasses = 4;   // 32 bits, most significant digit first
// A leaf's state between the passes: {prefix, rem} as int64. prefix holds the
// digits chosen so far in the key's top bits; rem is the weight still to be
// covered inside the prefix (>= 1), 0 for a leaf without weight (W = 0).
constexpr int kQselState = 2;

WH_QSEL_FN uint32_t qsel_bits(float r) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(r);
#else
  uint32_t b;
  std::memcpy(&b, &r, 4);
  return b;
#endif
}

WH_QSEL_FN float qsel_float(uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(b);
#else
  float r;
  std::memcpy(&r, &b, 4);
  return r;
#endif
}

// r -> a key with key(a) < key(b) iff a < b: the sign bit flipped for
// non-negatives, every bit for negatives; -0.0 is +0.0 first.
WH_QSEL_FN uint32_t qsel_key(float r) {
  uint32_t b = qsel_bits(r);
  if (b == 0x80000000u) b = 0;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

WH_QSEL_FN float qsel_unkey(uint32_t k) {
  return qsel_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// the fixed-point weight of a row: w * keep, rounded once (to nearest, ties to
// even) to a multiple of 1 / scale; scale a power of two
WH_QSEL_FN int64_t qsel_weight(float w, bool keep, double scale) {
  if (!keep || !(w > 0.f)) return 0;
  return (int64_t)rint((double)w * scale);
}

// the largest power of two 2^e (e in [-60, 100]) with total * 2^e <= 2^61:
// the rule of the histograms' scales
inline double qsel_scale(double total) {
  const double t = total > 1e-30 ? total : 1e-30;
  double e = std::floor(std::log2(0x1p61 / t));
  e = e < -60 ? -60 : (e > 100 ? 100 : e);
  return std::exp2(e);
}

// the weight the selected value has to reach: ceil(alpha * W) in fp64, kept
// within [1, W] (W > 0)
WH_QSEL_FN int64_t qsel_threshold(double alpha, int64_t W) {
  int64_t t = (int64_t)ceil(alpha * (double)W);
  if (t > W) t = W;
  return t < 1 ? 1 : t;
}

// pass p's digit of a key, and whether the key lies inside a prefix of p digits
WH_QSEL_FN int qsel_digit(uint32_t key, int pass) { return (int)(key >> (24 - 8 * pass)) & 255; }
WH_QSEL_FN bool qsel_match(uint32_t key, uint32_t prefix, int pass) {
  return pass == 0 || (key >> (32 - 8 * pass)) == (prefix >> (32 - 8 * pass));
}

// One pass's pick on a leaf's 256 global bins: the first digit d whose
// running sum reaches rem joins the prefix, the mass below it leaves rem.
// Pass 0 first turns the bins' total W into rem = qsel_threshold(alpha, W)
// (W = 0: the leaf is empty and stays so). False: the bins do not hold rem
// (inconsistent input), the state is left alone.
inline bool qsel_pick(const int64_t* bins, int pass, double alpha, int64_t* state) {
  int64_t rem = state[1];
  if (pass == 0) {
    int64_t W = 0;
    for (int d = 0; d < kQselBins; ++d) W += bins[d];
    state[0] = 0;
    state[1] = rem = W > 0 ? qsel_threshold(alpha, W) : 0;
  }
  if (rem <= 0) return true;
  int64_t below = 0;
  for (int d = 0; d < kQselBins; ++d) {
    if (below + bins[d] >= rem) {
      state[0] |= (int64_t)d << (24 - 8 * pass);
      state[1] = rem - below;
      return true;
    }
    below += bins[d];
  }
  return false;
}

// The histogram tasks of L leaf segments [beg[l], end[l]) of the key array,
// k_hist's task / reduce shape: a segment is cut into chunks of `chunk`
// positions, one block each,
//   tasks {leaf, begin, end}      red {leaf, first task, chunks}
// and an empty segment has neither (its bins stay zero). False: a segment
// outside [0, n], or begin > end.
inline bool qsel_plan(const std::vector<int64_t>& beg, const std::vector<int64_t>& end, int64_t n,
                      int64_t chunk, std::vector<int32_t>* tasks, std::vector<int32_t>* red) {
  if (beg.size() != end.size() || chunk < 1 || n > INT32_MAX) return false;
  for (size_t l = 0; l < beg.size(); ++l) {
    const int64_t b = beg[l], e = end[l];
    if (b < 0 || e < b || e > n) return false;
    if (e == b) continue;
    const int t0 = (int)(tasks->size() / 3);
    int nch = 0;
    for (int64_t r = b; r < e; r += chunk, ++nch)
      tasks->insert(tasks->end(), {(int32_t)l, (int32_t)r, (int32_t)(r + chunk < e ? r + chunk : e)});
    red->insert(red->end(), {(int32_t)l, t0, nch});
  }
  return true;
}

}  // namespace wh

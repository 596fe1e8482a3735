// The single-output objectives' gradient pairs, one small inline function per
// objective, shared by the gradient kernel (gbdt.hip k_gpair_obj<OBJ>) and the
// host (csrc/tests/host_selftest.cc evaluates them without a GPU). Everything
// is fp32, in the operation order of the plain-torch CPU path
// (models/gbdt_objective.py obj_gpair_torch), per unit of row weight: the
// caller multiplies by w -- except where `scaled` says the pair is final
// (binary:hinge's satisfied rows: g = 0, h = FLT_MIN whatever the weight).
// The table is docs/bsp_apps.md "Objectives and max_delta_step". exp is not
// guarded against margins beyond fp32's range (xgboost does not guard either).
// Free of torch; HIP only for the function qualifiers.
#pragma once

#include <cfloat>
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define WH_OBJ_FN __host__ __device__ __forceinline__
#else
#define WH_OBJ_FN inline
#endif

namespace wh {

// the ids of models/gbdt_objective.py OBJ_IDS
enum GbdtObj : int {
  kObjLogistic = 0,  // the logistic family under scale_pos_weight != 1
  kObjPoisson = 1,
  kObjGamma = 2,
  kObjTweedie = 3,
  kObjHinge = 4,
  kObjPseudoHuber = 5,
  kObjSquaredLog = 6,
  // (7 stays unassigned: the first id the gradient kernel refuses)
  kObjAbsolute = 8,  // reg:absoluteerror
  kObjQuantile = 9,  // reg:quantileerror, one output (its alpha in the scalars)
  kObjCount = 10
};

// the objectives' scalars, as they travel to the kernel
struct GbdtObjScalars {
  float max_delta_step;    // count:poisson: h = exp(m + max_delta_step)
  float tw1, tw2;          // reg:tweedie: 1 - rho and 2 - rho (tweedie_variance_power in (1, 2))
  float delta2;            // reg:pseudohubererror: huber_slope squared (> 0)
  float scale_pos_weight;  // the logistic family: rows with y == 1 weigh this much more
  float alpha = 0.5f;      // reg:quantileerror: the output's quantile, in (0, 1)
};

// (the differences and the square are taken in double and rounded once, as
// torch rounds a Python scalar that meets an fp32 tensor)
inline GbdtObjScalars gbdt_obj_scalars(double max_delta_step, double rho, double delta,
                                       double scale_pos_weight, double alpha = 0.5) {
  return {(float)max_delta_step, (float)(1.0 - rho), (float)(2.0 - rho), (float)(delta * delta),
          (float)scale_pos_weight, (float)alpha};
}

struct GbdtPair {
  float g, h;
  bool scaled;  // true: final, not to be multiplied by the row weight
};

constexpr float kSquaredLogMinMargin = (float)(-1.0 + 1e-6);

template <int OBJ>
WH_OBJ_FN GbdtPair gbdt_obj_pair(float m, float y, const GbdtObjScalars& a) {
  if constexpr (OBJ == kObjLogistic) {
    const float p = 1.f / (1.f + expf(-m));
    return {p - y, fmaxf(p * (1.f - p), 1e-16f), false};
  } else if constexpr (OBJ == kObjPoisson) {
    return {expf(m) - y, expf(m + a.max_delta_step), false};
  } else if constexpr (OBJ == kObjGamma) {
    const float r = y / expf(m);
    return {1.f - r, r, false};
  } else if constexpr (OBJ == kObjTweedie) {
    const float e1 = expf(a.tw1 * m), e2 = expf(a.tw2 * m);
    return {-y * e1 + e2, -y * a.tw1 * e1 + a.tw2 * e2, false};
  } else if constexpr (OBJ == kObjHinge) {
    const float ys = 2.f * y - 1.f;
    if (m * ys < 1.f) return {-ys, 1.f, false};
    return {0.f, FLT_MIN, true};
  } else if constexpr (OBJ == kObjPseudoHuber) {
    const float z = m - y, d2 = a.delta2;
    const float s = sqrtf(1.f + z * z / d2);
    return {z / s, d2 / ((d2 + z * z) * s), false};
  } else if constexpr (OBJ == kObjAbsolute) {  // h = w: no curvature, the leaves are refreshed
    const float d = m - y;
    return {d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f), 1.f, false};
  } else if constexpr (OBJ == kObjQuantile) {
    return {m - y >= 0.f ? 1.f - a.alpha : -a.alpha, 1.f, false};
  } else {
    static_assert(OBJ == kObjSquaredLog, "unknown objective id");
    const float mm = fmaxf(m, kSquaredLogMinMargin);
    const float lm = log1pf(mm), ly = log1pf(y), d = mm + 1.f;
    return {(lm - ly) / d, fmaxf((1.f - lm + ly) / (d * d), 1e-6f), false};
  }
}

// the row weight under scale_pos_weight (1 for every objective but the
// logistic family)
template <int OBJ>
WH_OBJ_FN float gbdt_obj_weight(float w, float y, const GbdtObjScalars& a) {
  if constexpr (OBJ == kObjLogistic) return y == 1.f ? w * a.scale_pos_weight : w;
  return w;
}

// The new metrics, per row and per unit of weight, in fp64 from the fp32
// inputs. link: how the objective turns a margin into its prediction.
enum GbdtLink : int { kLinkIdentity = 0, kLinkExp = 1, kLinkSigmoid = 2, kLinkStep = 3 };
enum GbdtMetric : int {
  kMetPoissonNll = 0,
  kMetGammaNll = 1,
  kMetGammaDeviance = 2,  // the sum; the metric is twice the mean
  kMetTweedieNll = 3,
  kMetMae = 4,
  kMetMphe = 5,
  kMetRmsle = 6,  // the squared log error; the metric is the root of the mean
  kMetCount = 7
};

WH_OBJ_FN double gbdt_link(int link, double m) {
  switch (link) {
    case kLinkExp: return exp(m);
    case kLinkSigmoid: return 1.0 / (1.0 + exp(-m));
    case kLinkStep: return m > 0.0 ? 1.0 : 0.0;
    default: return m;
  }
}

WH_OBJ_FN double gbdt_metric_loss(int metric, double p, double y, double rho, double delta) {
  switch (metric) {
    case kMetPoissonNll: {
      const double q = fmax(p, 1e-16);
      return lgamma(y + 1.0) + q - y * log(q);
    }
    case kMetGammaNll: {
      const double q = fmax(p, 1e-16);
      return y / q + log(q);
    }
    case kMetGammaDeviance: {
      const double q = p + 1e-16, t = y + 1e-16;
      return log(q / t) + t / q - 1.0;
    }
    case kMetTweedieNll:
      return -y * pow(p, 1.0 - rho) / (1.0 - rho) + pow(p, 2.0 - rho) / (2.0 - rho);
    case kMetMae: return fabs(p - y);
    case kMetMphe: {
      const double z = p - y, d2 = delta * delta;
      return d2 * (sqrt(1.0 + z * z / d2) - 1.0);
    }
    default: {
      const double d = log1p(y) - log1p(p);
      return d * d;
    }
  }
}

}  // namespace wh

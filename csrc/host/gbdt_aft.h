// survival:aft: the gradient pair and the loss of one row, small inline
// functions shared by the kernels (gbdt_survival.hip k_gpair_aft, k_aft_eval)
// and the host (csrc/tests/gbdt_survival_plan_test.cc evaluates them without
// a GPU), in the operation order of the plain-torch CPU path
// (models/gbdt_survival.py aft_gpair_torch). The row's interval is [yl, yu]
// (0 <= yl <= yu, yu may be inf), z(y) = (ln y - m) / sigma with ln 0 = -inf;
// yl == yu is an uncensored row. docs/bsp_apps.md "Survival" has the table.
//
// The forms are written so that they stay finite and accurate in the tails,
// and are evaluated in fp64 from the fp32 inputs; the pair is rounded to fp32
// once. (In fp32 the rounding of z alone costs a tail term like phi(z) or
// e^z a relative |z| 2^-24 and more; the kernel is bound by memory either way.)
//   normal     uncensored g = -z / s, h = 1 / s^2; censored through the Mills
//              ratio R(z) = (1 - Phi(z)) / phi(z) of the tail that holds the
//              interval (a scaled complementary error function), mirrored
//              for the lower tail, directly where the interval holds 0;
//   logistic   with F = sigmoid(z), S = sigmoid(-z): uncensored g = (S - F) / s,
//              h = 2 F S / s^2; censored g = (S_u - F_l) / s,
//              h = (F_u S_u + F_l S_l) / s^2 (ln(F_u - F_l) = ln F_u + ln S_l +
//              a term free of m);
//   extreme    with w = e^z, D = w_u - w_l, k = D / expm1(D): uncensored
//              g = (1 - w) / s, h = w / s^2; censored g = (k - w_l) / s,
//              h = (w_l + k (D / -expm1(-D) - 1)) / s^2.
// The result is clamped to xgboost's [-15, 15] and [1e-16, 15].
// Free of torch; HIP only for the function qualifiers.
#pragma once

#include <cmath>

#include "host/gbdt_objective.h"  // WH_OBJ_FN

namespace wh {

enum GbdtAftDist : int { kAftNormal = 0, kAftLogistic = 1, kAftExtreme = 2, kAftDistCount = 3 };

constexpr double kAftMinG = -15.0, kAftMaxG = 15.0, kAftMinH = 1e-16, kAftMaxH = 15.0;
constexpr double kAftEps = 1e-12;   // the metric's floor of the likelihood
constexpr double kAftMaxZ = 700.0;  // extreme: e^z stays finite

// exp(x^2) erfc(x) for x >= 0: the product while both factors are in range,
// then the asymptotic series (its next term is below 1e-8 there)
WH_OBJ_FN double aft_erfcx(double x) {
  if (x < 25.0) return exp(x * x) * erfc(x);
  const double i2 = 1.0 / (x * x);
  return (1.0 - 0.5 * i2 + 0.75 * i2 * i2) / (x * 1.7724538509055159);
}

// the Mills ratio (1 - Phi(z)) / phi(z) for z >= 0 (0 at inf)
WH_OBJ_FN double aft_mills(double z) {
  return 1.2533141373155001 * aft_erfcx(z * 0.70710678118654752);
}

WH_OBJ_FN double aft_phi(double z) { return 0.3989422804014327 * exp(-0.5 * z * z); }
WH_OBJ_FN double aft_sigmoid(double z) { return 1.0 / (1.0 + exp(-z)); }

// normal, the interval in the upper tail, 0 <= a < b <= inf:
// gs = sigma dl/dm, hs = sigma^2 d2l/dm2
WH_OBJ_FN void aft_normal_tail(double a, double b, double& gs, double& hs) {
  const double Ra = aft_mills(a), Rb = aft_mills(b);
  const double rho = exp(-0.5 * ((b - a) * (b + a)));  // phi(b) / phi(a)
  const double den = Ra - rho * Rb;
  const double brho = rho > 0.0 ? b * rho : 0.0;
  gs = (rho - 1.0) / den;
  hs = gs * gs - (a - brho) / den;
}

// gs = sigma dl/dm, hs = sigma^2 d2l/dm2 of a censored row, zl < zu
template <int DIST>
WH_OBJ_FN void aft_censored(double zl, double zu, double& gs, double& hs) {
  if constexpr (DIST == kAftNormal) {
    if (zl >= 0.0) {
      aft_normal_tail(zl, zu, gs, hs);
    } else if (zu <= 0.0) {
      aft_normal_tail(-zu, -zl, gs, hs);
      gs = -gs;
    } else {
      const double c = 0.70710678118654752;
      const double Fl = 0.5 * erfc(-zl * c), Qu = 0.5 * erfc(zu * c);
      const double den = 1.0 - Fl - Qu;
      const double pl = aft_phi(zl), pu = aft_phi(zu);
      const double zpl = pl > 0.0 ? zl * pl : 0.0, zpu = pu > 0.0 ? zu * pu : 0.0;
      gs = (pu - pl) / den;
      hs = gs * gs - (zpl - zpu) / den;
    }
  } else if constexpr (DIST == kAftLogistic) {
    const double Fl = aft_sigmoid(zl), Sl = aft_sigmoid(-zl);
    const double Fu = aft_sigmoid(zu), Su = aft_sigmoid(-zu);
    gs = Su - Fl;
    hs = Fu * Su + Fl * Sl;
  } else {
    static_assert(DIST == kAftExtreme, "unknown distribution");
    const double wl = exp(fmin(zl, kAftMaxZ)), wu = exp(fmin(zu, kAftMaxZ));
    const double D = wu - wl;
    const double k = D > 0.0 ? D / expm1(D) : 1.0;
    const double t = D > 0.0 ? D / -expm1(-D) : 1.0;
    gs = k - wl;
    hs = wl + k * (t - 1.0);
  }
}

template <int DIST>
WH_OBJ_FN void aft_uncensored(double z, double& gs, double& hs) {
  if constexpr (DIST == kAftNormal) {
    gs = -z;
    hs = 1.0;
  } else if constexpr (DIST == kAftLogistic) {
    const double F = aft_sigmoid(z), S = aft_sigmoid(-z);
    gs = S - F;
    hs = 2.0 * (F * S);
  } else {
    const double w = exp(fmin(z, kAftMaxZ));
    gs = 1.0 - w;
    hs = w;
  }
}

// the clamped pair per unit of row weight (fmax / fmin drop a NaN)
template <int DIST>
WH_OBJ_FN GbdtPair gbdt_aft_pair(float m, float yl, float yu, float sigma) {
  const double s = sigma, zl = (log((double)yl) - (double)m) / s;
  double gs, hs;
  if (yl == yu) {
    aft_uncensored<DIST>(zl, gs, hs);
  } else {
    aft_censored<DIST>(zl, (log((double)yu) - (double)m) / s, gs, hs);
  }
  const double g = gs / s, h = hs / (s * s);
  return {(float)fmin(fmax(g, kAftMinG), kAftMaxG), (float)fmin(fmax(h, kAftMinH), kAftMaxH),
          false};
}

// -ln max(likelihood, 1e-12) of a row, in fp64 from the fp32 inputs
WH_OBJ_FN double gbdt_aft_loss(int dist, double m, double yl, double yu, double sigma) {
  const double zl = (log(yl) - m) / sigma;
  double lik;
  if (yl == yu) {
    double f;
    if (dist == kAftNormal) {
      f = 0.3989422804014327 * exp(-0.5 * zl * zl);
    } else if (dist == kAftLogistic) {
      f = (1.0 / (1.0 + exp(-zl))) * (1.0 / (1.0 + exp(zl)));
    } else {
      const double w = exp(zl);
      f = w < 1e300 ? w * exp(-w) : 0.0;
    }
    lik = f / (sigma * yl);
  } else {
    const double zu = (log(yu) - m) / sigma;
    if (dist == kAftNormal) {
      const double c = 0.70710678118654752;
      if (zl >= 0.0) lik = 0.5 * (erfc(zl * c) - erfc(zu * c));
      else if (zu <= 0.0) lik = 0.5 * (erfc(-zu * c) - erfc(-zl * c));
      else lik = 1.0 - 0.5 * erfc(zu * c) - 0.5 * erfc(-zl * c);
    } else if (dist == kAftLogistic) {
      lik = (1.0 / (1.0 + exp(-zu))) * (1.0 / (1.0 + exp(zl))) * -expm1(-(zu - zl));
    } else {
      const double wl = exp(zl), wu = exp(zu);
      lik = wl < 1e300 ? exp(-wl) * -expm1(-(wu - wl)) : 0.0;
    }
  }
  return -log(fmax(lik, kAftEps));
}

}  // namespace wh

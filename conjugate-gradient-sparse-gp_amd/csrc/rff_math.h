// rff_math.h -- the phase arithmetic of the random-Fourier-feature kernels, shared by rff.hip (features, prior
// samples) and rff_grad.hip (their VJP), so that the backward pass sees exactly the phases of the forward pass.
//
// Phases are kept in revolutions: t = sum_d x_d theta'_d with theta' = theta / (2 pi), r = t - rint(t) is exact, and
// one sin/cos polynomial pair on [-pi/4, pi/4] after a quadrant split replaces libm sin/cos per feature.
//
// Error of a feature (fp64, u = 2^-53): |sin - sin(theta_l . x_n)|, |cos - ...| <= 8 u (1 + sum_d |x_d theta_d|):
// theta' carries 1 u relative, each of the D products and fmas of the chain at most 1 u of sum_d |x_d theta'_d|
// revolutions, i.e. 2 pi times that in radians -- together below 7 u sum_d |x_d theta_d| (2 pi < 6.3, plus the
// rounding of theta') -- and the argument scaling, the polynomials (truncation < 5e-17) and their Horner chains less
// than 8 u on values of modulus <= 1.
#pragma once

#include "mgp_math.h"

// sin(2 pi r), cos(2 pi r) for r in [-1/2, 1/2] revolutions: quadrant q = rint(4 r), f = r - q/4 in [-1/8, 1/8] (both
// steps exact), a = 2 pi f in [-pi/4, pi/4], Taylor polynomials in a^2 (fp64: through a^15 / a^16, truncation
// < 5e-17; fp32: through a^9 / a^10, < 2e-9), then the quadrant rotation.
__device__ __forceinline__ void rff_sincos_poly(double a, double& s, double& c) {
  const double a2 = a * a;
  double ps = -7.6471637318198164759e-13;            // -1/15!
  ps = mgp_fma(ps, a2, 1.6059043836821614599e-10);   // 1/13!
  ps = mgp_fma(ps, a2, -2.5052108385441718775e-08);  // -1/11!
  ps = mgp_fma(ps, a2, 2.7557319223985890653e-06);   // 1/9!
  ps = mgp_fma(ps, a2, -1.9841269841269841270e-04);  // -1/7!
  ps = mgp_fma(ps, a2, 8.3333333333333333333e-03);   // 1/5!
  ps = mgp_fma(ps, a2, -1.6666666666666666667e-01);  // -1/3!
  s = mgp_fma(ps * a2, a, a);
  double pc = 4.7794773323873852974e-14;             // 1/16!
  pc = mgp_fma(pc, a2, -1.1470745597729724714e-11);  // -1/14!
  pc = mgp_fma(pc, a2, 2.0876756987868098979e-09);   // 1/12!
  pc = mgp_fma(pc, a2, -2.7557319223985890653e-07);  // -1/10!
  pc = mgp_fma(pc, a2, 2.4801587301587301587e-05);   // 1/8!
  pc = mgp_fma(pc, a2, -1.3888888888888888889e-03);  // -1/6!
  pc = mgp_fma(pc, a2, 4.1666666666666666667e-02);   // 1/4!
  pc = mgp_fma(pc, a2, -0.5);
  c = mgp_fma(pc, a2, 1.0);
}
__device__ __forceinline__ void rff_sincos_poly(float a, float& s, float& c) {
  const float a2 = a * a;
  float ps = 2.7557319e-06f;               // 1/9!
  ps = mgp_fma(ps, a2, -1.9841270e-04f);  // -1/7!
  ps = mgp_fma(ps, a2, 8.3333333e-03f);   // 1/5!
  ps = mgp_fma(ps, a2, -1.6666667e-01f);  // -1/3!
  s = mgp_fma(ps * a2, a, a);
  float pc = -2.7557319e-07f;              // -1/10!
  pc = mgp_fma(pc, a2, 2.4801587e-05f);   // 1/8!
  pc = mgp_fma(pc, a2, -1.3888889e-03f);  // -1/6!
  pc = mgp_fma(pc, a2, 4.1666667e-02f);   // 1/4!
  pc = mgp_fma(pc, a2, -0.5f);
  c = mgp_fma(pc, a2, 1.0f);
}

template <typename T>
__device__ __forceinline__ void rff_sincos_rev(T t, T& s, T& c) {
  const T r = t - __builtin_rint(t);
  const T qf = __builtin_rint(r * (T)4);
  const T f = mgp_fma(qf, (T)-0.25, r);
  T sa, ca;
  rff_sincos_poly(f * (T)6.283185307179586476925, sa, ca);
  const int q = (int)qf & 3;  // -2..2 -> 2, 3, 0, 1, 2
  const T s1 = (q & 1) ? ca : sa;
  const T c1 = (q & 1) ? sa : ca;
  s = (q & 2) ? -s1 : s1;
  c = ((q + 1) & 2) ? -c1 : c1;
}

// The per-entry formulas of a stationary primitive in terms of the squared scaled distance q2: its value, d k / d q2 and RatQuad's
// d k / d alpha (kernels.py:436-439, 467-471, 560-610; Stationary.euclid_dist's sqrt(r2 + 1e-12), :424-426).  One copy for the
// dense gradient kernels (grad_common.hpp includes this) and the matrix-free gradient form (kmvm.hip).  Every expression keeps the
// grouping it had in grad_common.hpp: the compiler contracts multiply-adds by expression shape.
#pragma once
#include "gps_common.hpp"
#include <cmath>

#define GRAD_SQRT3 1.7320508075688772
#define GRAD_SQRT5 2.23606797749979

// stationary primitive from the squared scaled distance q2 (alpha: RatQuad's).  EXT == false: a kernel instance that is never
// handed RatQuad (grad.hip keeps one such instance, with the code it had before that primitive existed)
template <bool EXT = true>
__device__ __forceinline__ double grad_stationary_value(int op, double variance, double q2, double alpha) {
  if (op == GPS_K_RBF) return variance * exp(-q2 / 2.0);
  if (EXT && op == GPS_K_RATQUAD) return variance * exp(-alpha * log1p(0.5 * q2 * (1.0 / alpha)));    // (1 + q2 / (2 alpha))^-alpha
  const double sq3 = GRAD_SQRT3, sq5 = GRAD_SQRT5;
  const double rad = sqrt(q2 + 1e-12);
  if (op == GPS_K_MATERN12) return variance * exp(-rad);
  if (op == GPS_K_EXPONENTIAL) return variance * exp(-0.5 * rad);
  if (op == GPS_K_MATERN32) return variance * (1.0 + sq3 * rad) * exp(-sq3 * rad);
  return variance * (1.0 + sq5 * rad + 5.0 / 3.0 * (rad * rad)) * exp(-sq5 * rad);
}

// d k / d (q2) of a stationary primitive with value k at squared scaled distance q2
template <bool EXT = true>
__device__ __forceinline__ double grad_dk_dq2(int op, double variance, double k, double q2, double alpha) {
  if (op == GPS_K_RBF) return -0.5 * k;
  if (EXT && op == GPS_K_RATQUAD) return -0.5 * k / (1.0 + 0.5 * q2 / alpha);
  const double sq3 = GRAD_SQRT3, sq5 = GRAD_SQRT5;
  const double rad = sqrt(q2 + 1e-12);
  if (op == GPS_K_MATERN12) return -k / (2.0 * rad);
  if (op == GPS_K_EXPONENTIAL) return -k / (4.0 * rad);
  if (op == GPS_K_MATERN32) return -1.5 * variance * exp(-sq3 * rad);
  return -(5.0 / 6.0) * variance * (1.0 + sq5 * rad) * exp(-sq5 * rad);
}

// d k / d alpha of RatQuad with value k:  k (t / (1 + t) - log1p(t)),  t = q2 / (2 alpha)
__device__ __forceinline__ double grad_ratquad_dalpha(double k, double q2, double alpha) {
  const double t = 0.5 * q2 / alpha;
  return k * (t / (1.0 + t) - log1p(t));
}

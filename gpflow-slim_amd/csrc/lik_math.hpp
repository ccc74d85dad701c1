// Special functions of the likelihood kernels (lik.hip) that libm / the device library do not have.  Usable from host and
// device code; a plain C++ compiler sees no qualifiers (tests/cpu_lik/digamma_main.cpp compiles this header on its own).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPS_LIK_HD __host__ __device__
#else
#define GPS_LIK_HD
#endif

// psi(x) = d log Gamma(x) / dx for x > 0 (densities.beta / densities.gamma differentiated: Beta per quadrature node, Gamma and
// Beta once per call).  The argument is shifted up with psi(x) = psi(x + 1) - 1 / x until x >= 10; there the asymptotic series
// ln x - 1 / (2 x) - sum_k B_2k / (2 k x^2k)  through x^-14 (the first term left out is 3617 / (8160 x^16) < 4.5e-17).
// The shift is a data-dependent loop of at most ten steps.  A form with uniform control flow (always ten steps as ONE quotient
// num / den built with nine fused multiply-adds, dropped by a select where x >= 10) was tried for the device, where lanes of
// one wavefront see alpha = m s from 1e-4 to 1e2 side by side: it was 9 % slower in the Beta launch (1.21 ms against 1.11 ms at
// N = 1e6, docs/LAB_NOTES.md) -- the loop costs a wavefront its slowest lane, which is what the uniform form costs every lane.
GPS_LIK_HD inline double digamma(double x) {
  double shift = 0.0;
  while (x < 10.0) { shift += 1.0 / x; x += 1.0; }
  const double r = 1.0 / x, r2 = r * r;
  // B_2k / (2 k), k = 1 .. 7:  1/12, -1/120, 1/252, -1/240, 1/132, -691/32760, 1/12
  const double tail = r2 * (1.0 / 12.0 - r2 * (1.0 / 120.0 - r2 * (1.0 / 252.0 - r2 * (1.0 / 240.0 - r2 * (1.0 / 132.0 -
                      r2 * (691.0 / 32760.0 - r2 * (1.0 / 12.0)))))));
  return ((log(x) - 0.5 * r) - tail) - shift;
}

// kmat_prim_value's formulas (kmat_common.hpp) restated for float, for the fp32 fused product of kmvm_f32.hip: the value of a
// stationary primitive from its dot product and the two squared norms.  One copy, as there.
//
// What differs from the fp64 form is the transcendental path, not the formulas: the exponential is the hardware's exp2 (v_exp_f32)
// with the log2 e prescale folded into the constant the host prepares, the square root is v_sqrt_f32, and RatQuad's power is
// exp2(-alpha log2(1 + t)) on v_log_f32 -- each about 1 ulp of a float, beside the 2^-24 |x log2 e| the argument's own rounding
// leaves in exp(x).  The clamp of r2 at 0 keeps a NaN (kernels.py:421), sqrt(r2 + 1e-12) keeps its epsilon.
#pragma once
#include "kmat_common.hpp"

#define GPS_LOG2E_F 1.44269504088896340736f

// the primitive as the fp32 epilogue reads it (host side: kmat_node_f32)
//   RBF: e0 = -0.5 log2 e ; Matern12: e0 = -log2 e ; Exponential: e0 = -0.5 log2 e (on r) ; Matern32: c0 = sqrt 3, e0 = -sqrt 3 log2 e ;
//   Matern52: c0 = sqrt 5, e0 = -sqrt 5 log2 e ; RatQuad: c0 = 0.5 / alpha, e0 = -alpha
struct KNodeF32 { float variance, c0, e0; };

static inline KNodeF32 kmat_node_f32(const KNodeDev& nd) {
  KNodeF32 o;
  o.variance = (float)nd.variance; o.c0 = 0.0f; o.e0 = 0.0f;
  const double l2e = 1.4426950408889634;
  switch (nd.op) {
    case GPS_K_RBF: case GPS_K_EXPONENTIAL: o.e0 = (float)(-0.5 * l2e); break;
    case GPS_K_MATERN12: o.e0 = (float)(-l2e); break;
    case GPS_K_MATERN32: o.c0 = (float)sqrt(3.0); o.e0 = (float)(-sqrt(3.0) * l2e); break;
    case GPS_K_MATERN52: o.c0 = (float)sqrt(5.0); o.e0 = (float)(-sqrt(5.0) * l2e); break;
    case GPS_K_RATQUAD: o.c0 = (float)(0.5 * nd.c1); o.e0 = (float)(-nd.c0); break;
    default: break;
  }
  return o;
}

#if defined(__HIPCC__)
__device__ __forceinline__ float gps_clamp0_f32(float r2) { return (r2 < 0.0f) ? 0.0f : r2; }

template <int OP>
__device__ __forceinline__ float kmat_prim_value_f32(const KNodeF32& nd, float dot, float ni, float nj) {
  float r2 = -2.0f * dot + (ni + nj);
  r2 = gps_clamp0_f32(r2);
  if (OP == GPS_K_RBF) return nd.variance * __builtin_amdgcn_exp2f(nd.e0 * r2);
  if (OP == GPS_K_RATQUAD) return nd.variance * __builtin_amdgcn_exp2f(nd.e0 * __builtin_amdgcn_logf(1.0f + nd.c0 * r2));
  const float r = __builtin_amdgcn_sqrtf(r2 + 1e-12f);
  const float e = __builtin_amdgcn_exp2f(nd.e0 * r);
  if (OP == GPS_K_MATERN12 || OP == GPS_K_EXPONENTIAL) return nd.variance * e;
  if (OP == GPS_K_MATERN32) return nd.variance * (1.0f + nd.c0 * r) * e;
  return nd.variance * (1.0f + nd.c0 * r + (5.0f / 3.0f) * (r * r)) * e;
}
#endif

// The pieces of the fisheye lens model (include/pf_hip.h, the lens model; DESIGN.md sections 30 and 33) that both directions need, each written once:
// the `on` test of a lens row, the Kannala-Brandt polynomial and its derivative, rho with its inverse and its derivative.  fisheye_target.hip
// (pixel -> direction) includes this file; fisheye_gather.hip (direction -> pixel) keeps its own text of the `on` test, the polynomial and rho, which
// are these expressions letter for letter, so that its kernels stay the instructions they were measured with.
// Every rounding step is spelled out (contraction off, fmaf where a fused step is meant): the bits must not depend on the kernel they are inlined into.
#pragma once

#include <math.h>

#include "../../include/pf_hip.h"
#include "cam_model.h"

namespace pf {

// a lens is on iff its 12 entries are finite and theta_max > 0
__device__ __forceinline__ bool fisheye_lens_on(const float* __restrict__ lens) {
  return all_finite(lens, PF_FISHEYE_LENS_FLOATS) && lens[6] > 0.f;
}

// P(t) = t (1 + t^2 (k1 + t^2 (k2 + t^2 (k3 + t^2 k4)))), Horner-wise
__device__ __forceinline__ float fisheye_poly(float t, float k1, float k2, float k3, float k4) {
#pragma clang fp contract(off)
  const float t2 = t * t;
  return t * fmaf(t2, fmaf(t2, fmaf(t2, fmaf(t2, k4, k3), k2), k1), 1.f);
}

// P'(t) = 1 + t^2 (3 k1 + t^2 (5 k2 + t^2 (7 k3 + 9 k4 t^2)))
__device__ __forceinline__ float fisheye_poly_slope(float t, float k1, float k2, float k3, float k4) {
#pragma clang fp contract(off)
  const float t2 = t * t;
  return fmaf(t2, fmaf(t2, fmaf(t2, fmaf(t2, 9.f * k4, 7.f * k3), 5.f * k2), 3.f * k1), 1.f);
}

// rho(td): td | 2 sin(td / 2) | 2 tan(td / 2)
__device__ __forceinline__ float fisheye_rho(int kind, float td) {
#pragma clang fp contract(off)
  return kind == PF_FISHEYE_EQUIDISTANT ? td : kind == PF_FISHEYE_EQUISOLID ? 2.f * sinf(td * 0.5f) : 2.f * tanf(td * 0.5f);
}

// its inverse: rho | 2 asin(min(rho / 2, 1)) | 2 atan(rho / 2); the minimum keeps a rho that rounding has taken past 2 inside asin's domain
__device__ __forceinline__ float fisheye_rho_inverse(int kind, float rho) {
#pragma clang fp contract(off)
  return kind == PF_FISHEYE_EQUIDISTANT ? rho : kind == PF_FISHEYE_EQUISOLID ? 2.f * asinf(fminf(rho * 0.5f, 1.f)) : 2.f * atanf(rho * 0.5f);
}

// rho'(td): 1 | cos(td / 2) | 1 / cos^2(td / 2)
__device__ __forceinline__ float fisheye_rho_slope(int kind, float td) {
#pragma clang fp contract(off)
  if (kind == PF_FISHEYE_EQUIDISTANT) return 1.f;
  const float c = cosf(td * 0.5f);
  return kind == PF_FISHEYE_EQUISOLID ? c : 1.f / (c * c);
}

// The same functions over the dual numbers T of fit_dual.h (the lens fit, fit_camera_fisheye.hip), with k3 = k4 = 0 and the kind at
// compile time.  Templates, so a unit that does not instantiate them carries nothing of them; dsincos, dasin, datan and recip are found where T is.
template <class T>
__device__ __forceinline__ T fisheye_poly_slope(const T& t, const T& k1, const T& k2) {
  const T t2 = t * t;
  return t2 * (k1 * 3.f + t2 * (k2 * 5.f)) + 1.f;
}

// the caller has made sure that rho < 2 for the equisolid kind
template <int KIND, class T>
__device__ __forceinline__ T fisheye_rho_inverse(const T& rho) {
  if constexpr (KIND == PF_FISHEYE_EQUIDISTANT) return rho;
  else if constexpr (KIND == PF_FISHEYE_EQUISOLID) return dasin(rho * 0.5f) * 2.f;
  else return datan(rho * 0.5f) * 2.f;
}

// rho'(td) of the two kinds where it is not 1
template <int KIND, class T>
__device__ __forceinline__ T fisheye_rho_slope(const T& td) {
  static_assert(KIND == PF_FISHEYE_EQUISOLID || KIND == PF_FISHEYE_STEREOGRAPHIC, "rho' = 1 for the equidistant kind");
  T s, c;
  dsincos(td * 0.5f, &s, &c);
  if constexpr (KIND == PF_FISHEYE_EQUISOLID) return c;
  else return recip(c * c);
}

}  // namespace pf

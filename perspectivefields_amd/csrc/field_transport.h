// The differential of the Unified Spherical Model projection (pinhole at xi = 0) in closed form, shared by the two kernels of field_transport.hip: an up
// vector is a tangent direction, and it moves between image planes through (unproject, rotate, project).  No finite differences and no dual numbers
// (fit_dual.h): the closed form below is two dot products and four multiply-adds per push, and tests/test_field_transport_ref.py states the same form in
// fp64.  Gravity does not enter: only the ray X and the tangent t at it.
// No PF_NO_PK_F32 here: field_transport.hip is compiled without packed fp32 as a whole (build.py NO_PK_F32_FLAGS).
#pragma once

#include "cam_model.h"

namespace pf {

// image direction (not normalised) of the tangent t at the ray X (any length) under (X.x, X.y) / (X.z + xi |X|): the derivative along t times D^2,
//   (t.x D - X.x s, t.y D - X.y s), D = X.z + xi |X|, s = t.z + xi (X . t) / |X|
// D > 0 on the rays the camera sees (usm_z_min), so the factor D^2 keeps the direction.  usm_up_of_ray (cam_model.h) is this for t = g, |X| = 1
__device__ __forceinline__ void usm_push(const float* X, const float* t, float xi, float* px, float* py) {
  const float n = sqrtf(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
  const float D = X[2] + xi * n;
  const float s = t[2] + xi * (X[0] * t[0] + X[1] * t[1] + X[2] * t[2]) / n;
  *px = t[0] * D - X[0] * s;
  *py = t[1] * D - X[1] * s;
}

// the unit tangent t, t . X = 0, whose usm_push is a positive multiple of m = (mx, my).  Orthonormal basis of the tangent plane: e1 = (X x h) / |X x h|
// with h = (1, 0, 0) where |X.x| < 0.9 |X|, else (0, 1, 0); e2 = (X / |X|) x e1.  With p_k = usm_push(e_k) the 2 x 2 system alpha p_1 + beta p_2 = m
// is solved by Cramer's rule up to its determinant, whose sign alone is applied: (alpha, beta) is then scaled to unit length.  The projection is a
// local diffeomorphism on the rays a camera sees, so the determinant does not vanish there; a zero or NaN solution gives NaN, which every later
// (positive) comparison rejects
__device__ __forceinline__ void usm_lift(const float* X, float mx, float my, float xi, float* t) {
  const float n = sqrtf(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
  const float inv = 1.f / n;
  const float x0 = X[0] * inv, x1 = X[1] * inv, x2 = X[2] * inv;
  float e1[3], e2[3];
  if (fabsf(X[0]) < 0.9f * n) {  // X x (1, 0, 0) = (0, X.z, -X.y)
    const float k = 1.f / sqrtf(x2 * x2 + x1 * x1);
    e1[0] = 0.f; e1[1] = x2 * k; e1[2] = -x1 * k;
  } else {  // X x (0, 1, 0) = (-X.z, 0, X.x)
    const float k = 1.f / sqrtf(x2 * x2 + x0 * x0);
    e1[0] = -x2 * k; e1[1] = 0.f; e1[2] = x0 * k;
  }
  e2[0] = x1 * e1[2] - x2 * e1[1];
  e2[1] = x2 * e1[0] - x0 * e1[2];
  e2[2] = x0 * e1[1] - x1 * e1[0];
  float p1x, p1y, p2x, p2y;
  usm_push(X, e1, xi, &p1x, &p1y);
  usm_push(X, e2, xi, &p2x, &p2y);
  const float sg = copysignf(1.f, p1x * p2y - p1y * p2x);
  const float al = (mx * p2y - my * p2x) * sg, be = (p1x * my - p1y * mx) * sg;
  const float k = 1.f / sqrtf(al * al + be * be);
  t[0] = (al * e1[0] + be * e2[0]) * k;
  t[1] = (al * e1[1] + be * e2[1]) * k;
  t[2] = (al * e1[2] + be * e2[2]) * k;
}

// X = M^T v for a row-major 3 x 3 matrix
__device__ __forceinline__ void rotate_t(const float* M, const float* v, float* X) {
  X[0] = M[0] * v[0] + M[3] * v[1] + M[6] * v[2];
  X[1] = M[1] * v[0] + M[4] * v[1] + M[7] * v[2];
  X[2] = M[2] * v[0] + M[5] * v[1] + M[8] * v[2];
}

}  // namespace pf

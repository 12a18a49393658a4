// The per-pixel error between a predicted and a ground-truth perspective field (include/pf_hip.h pf_field_errors): ONE function, so that
// every kernel that computes an error gives the same bits for the same six inputs -- the radix selection of field_err.hip compares bit
// patterns across passes.  Every rounding step is spelled out (contraction off, fmaf where a fused step is meant), as in cam_model.h.
#pragma once

#include "pf_kernels.h"

namespace pf {

struct FieldErr {
  float up, lat;  // degrees; NaN where the pixel is invalid
  bool valid;
};

__device__ __forceinline__ PF_NO_PK_F32 FieldErr field_error_at(float px, float py, float gx, float gy, float lp, float lg) {
#pragma clang fp contract(off)
  // both products rounded, no fused step: the cross product of a vector with itself (or a multiple by a power of two) is exactly 0
  const float cr = fabsf(px * gy - py * gx);
  const float dt = px * gx + py * gy;
  const float dl = fabsf(lp - lg);
  const float p2 = fmaf(px, px, py * py), g2 = fmaf(gx, gx, gy * gy);
  FieldErr e;
  // a finite squared length means finite components; a non-finite latitude makes dl non-finite
  e.valid = p2 >= 1e-12f && g2 >= 1e-12f && p2 < INFINITY && g2 < INFINITY && cr < INFINITY && fabsf(dt) < INFINITY && dl < INFINITY;
  e.up = e.valid ? fminf(atan2f(cr, dt) * 57.29577951308232f, 180.f) : NAN;  // fp32 pi * 180 / pi may round above 180
  e.lat = e.valid ? dl : NAN;
  return e;
}

}  // namespace pf

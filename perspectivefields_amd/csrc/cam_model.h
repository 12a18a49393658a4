// Camera parameters -> perspective fields at one pixel.  Pinhole: the per-pixel body of fields_from_params_kernel (elem.hip),
// shared with the pinhole (xi = 0) labels of pano_crop.hip so that both give the same bits for the same fp32 parameters.
// Reference: PanoCam.get_up_general / get_lat_general (utils/panocam.py:451-556).  Quirks kept: up vectors at pixel centres
// (j + 0.5); latitude on linspace(-c, size - c, size) (end points included); elevation == 0 -> constant up field.
// PF_NO_PK_F32 on both pinhole helpers: they inline into kernels compiled without the packed-fp32 feature (pf_kernels.h).
#pragma once

#include "pf_kernels.h"

namespace pf {

struct PinholeFields {
  float sr, cr, se, ce, f, cx, cy, sx, sy, vx, vy, sgn, el;
};

// roll, el (elevation = pitch) in radians; rel_f, rel_cx, rel_cy as in pf_fields_from_params
__device__ __forceinline__ PF_NO_PK_F32 PinholeFields pinhole_fields_setup(float roll, float el, float rel_f, float rel_cx, float rel_cy, int H, int W) {
#pragma clang fp contract(off)
  PinholeFields c;
  c.el = el;
  c.f = rel_f * (float)H;
  c.cx = (rel_cx + 0.5f) * (float)W;
  c.cy = (rel_cy + 0.5f) * (float)H;
  sincosf(roll, &c.sr, &c.cr);
  sincosf(el, &c.se, &c.ce);
  c.sx = W > 1 ? (float)W / (float)(W - 1) : 0.f;
  c.sy = H > 1 ? (float)H / (float)(H - 1) : 0.f;
  c.vx = el != 0.f ? c.sr * c.ce * c.f / -c.se + c.cx : 0.f;
  c.vy = el != 0.f ? c.cr * c.ce * c.f / -c.se + c.cy : 0.f;
  c.sgn = el > 0.f ? 1.f : -1.f;
  return c;
}

struct FieldsPixel {
  float ux, uy, lat;
};
// up field (ux, uy) and latitude (degrees) of pixel (row, col).  Every rounding step is spelled out (contraction off, fmaf where
// the compiler had contracted): the bits must not depend on the kernel this is inlined into.
__device__ __forceinline__ PF_NO_PK_F32 FieldsPixel pinhole_fields_at(const PinholeFields& c, int row, int col) {
#pragma clang fp contract(off)
  float ux, uy;
  if (c.el == 0.f) { ux = -c.sr; uy = -c.cr; }
  else { ux = (c.vx - ((float)col + 0.5f)) * c.sgn; uy = (c.vy - ((float)row + 0.5f)) * c.sgn; }
  const float inv = 1.0f / sqrtf(fmaf(uy, uy, ux * ux));
  FieldsPixel o;
  o.ux = ux * inv;
  o.uy = uy * inv;
  const float x = fmaf((float)col, c.sx, -c.cx) / c.f, y = fmaf((float)row, c.sy, -c.cy) / c.f;
  const float xw = fmaf(x, c.cr, -(y * c.sr));
  const float yw = fmaf(y * c.ce, c.cr, x * c.ce * c.sr) - c.se;
  const float zw = fmaf(y * c.se, c.cr, x * c.se * c.sr) + c.ce;
  o.lat = -atan2f(yw, sqrtf(fmaf(xw, xw, zw * zw))) * 57.29577951308232f;
  return o;
}

// ---------------------------------------------------------------- Unified Spherical Model labels (xi != 0), shared by pano_crop.hip and
// fields_usm_kernel (fit_camera_usm.hip) so that both give the same bits.  R = R_pitch R_roll, camera -> world, row major; g = R^T (0, -1, 0).
// The formulas are split from the test disc >= 0 so that each kernel keeps its own branches (with them, its instructions).
// No PF_NO_PK_F32 here: both units that use these helpers are compiled without packed fp32 as a whole (build.py NO_PK_F32_FLAGS).
// rho^2 and disc of the image point (x, y) = ((a - Cx) / F, (b - Cy) / F); the point has a ray where disc >= 0
__device__ __forceinline__ float usm_disc(float x, float y, float xi, float* r2) {
  *r2 = x * x + y * y;
  return 1.f + (1.f - xi * xi) * *r2;
}
// its ray X, given disc >= 0
__device__ __forceinline__ void usm_ray_of(float x, float y, float xi, float r2, float disc, float* X) {
  const float eta = (xi + sqrtf(disc)) / (1.f + r2);
  X[0] = eta * x;
  X[1] = eta * y;
  X[2] = eta - xi;
}
// both: false where the point has no ray
__device__ __forceinline__ bool usm_ray(float x, float y, float xi, float* X) {
  float r2;
  const float disc = usm_disc(x, y, xi, &r2);
  if (!(disc >= 0.f)) return false;
  usm_ray_of(x, y, xi, r2, disc, X);
  return true;
}

// the inverse: the normalised image point (x, y) of a ray X of any length, (X_x, X_y) / (X_z + xi |X|).  usm_ray's "+" root gives exactly the
// rays with X_z > usm_z_min(xi) |X|; on those the denominator is positive and usm_project(usm_ray(x, y)) = (x, y)
__device__ __forceinline__ void usm_project(const float* X, float xi, float* x, float* y) {
  const float D = X[2] + xi * sqrtf(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
  *x = X[0] / D;
  *y = X[1] / D;
}
// lower bound (exclusive) of X_z of a unit ray that the camera sees: -xi for xi <= 1 (0 for the pinhole camera), -1 / xi beyond; NaN for a NaN xi
__device__ __forceinline__ float usm_z_min(float xi) { return xi > 1.f ? -1.f / xi : 0.f - xi; }

// camera -> world, R = R_pitch(p) R_roll(r), row major, from the sines and cosines of roll and pitch
__device__ __forceinline__ void cam_rotation(float sr, float cr, float sp, float cp, float* R) {
  R[0] = cr; R[1] = -sr; R[2] = 0.f;
  R[3] = cp * sr; R[4] = cp * cr; R[5] = -sp;
  R[6] = sp * sr; R[7] = sp * cr; R[8] = cp;
}
__device__ __forceinline__ void cam_rotation(float roll, float pitch, float* R) {
  float sr, cr, sp, cp;
  sincosf(roll, &sr, &cr);
  sincosf(pitch, &sp, &cp);
  cam_rotation(sr, cr, sp, cp, R);
}

__device__ __forceinline__ void to_world(const float* R, const float* X, float* Xw) {
  Xw[0] = R[0] * X[0] + R[1] * X[1] + R[2] * X[2];
  Xw[1] = R[3] * X[0] + R[4] * X[1] + R[5] * X[2];
  Xw[2] = R[6] * X[0] + R[7] * X[1] + R[8] * X[2];
}

// up vector at a pixel centre whose ray is X
__device__ __forceinline__ void usm_up_of_ray(const float* X, const float* g, float xi, float* ux, float* uy) {
  const float D = X[2] + xi;
  const float s = g[2] + xi * (X[0] * g[0] + X[1] * g[1] + X[2] * g[2]);
  const float a = g[0] * D - X[0] * s, b = g[1] * D - X[1] * s;
  const float inv = 1.f / sqrtf(a * a + b * b);
  *ux = a * inv;
  *uy = b * inv;
}

// latitude (degrees) of the ray X of a linspace point
__device__ __forceinline__ float usm_lat_of_ray(const float* X, const float* R) {
  float Xw[3];
  to_world(R, X, Xw);
  return -atan2f(Xw[1], sqrtf(Xw[0] * Xw[0] + Xw[2] * Xw[2])) * 57.29577951308232f;
}

}  // namespace pf

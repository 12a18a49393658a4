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

// ---------------------------------------------------------------- Model pieces of the supersampled gathers (gather_ss.h), each written once.  Every
// rounding step is spelled out (contraction off, fmaf where a fused step is meant): the bits must not depend on the kernel they are inlined into.
// pano_rotate.hip calls pano_rotation (its kernels compile to the same instructions with it) and keeps its own pixel ->
// direction inside its rot_pixel, which has no sub-sample offset.
__device__ __forceinline__ bool all_finite(const float* p, int n) {
  bool fin = true;
  for (int k = 0; k < n; ++k) fin = fin && isfinite(p[k]);
  return fin;
}

// Q = Y(yaw) R_pitch(pitch) R_roll(roll), camera -> world, row major; Y = [[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]
__device__ __forceinline__ void world_rotation(float roll, float pitch, float yaw, float* Q) {
#pragma clang fp contract(off)
  float R[9], sy, cy;
  cam_rotation(roll, pitch, R);
  sincosf(yaw, &sy, &cy);
  for (int k = 0; k < 3; ++k) {
    Q[k] = fmaf(cy, R[k], sy * R[6 + k]);
    Q[3 + k] = R[3 + k];
    Q[6 + k] = fmaf(cy, R[6 + k], -(sy * R[k]));
  }
}
// A = Q of rot = {roll, pitch, yaw}, or Q^T with `inverse`: output direction -> world direction of a rotated panorama
__device__ __forceinline__ void pano_rotation(const float* rot, int inverse, float* A) {
  float Q[9];
  world_rotation(rot[0], rot[1], rot[2], Q);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[3 * i + j] = inverse ? Q[3 * j + i] : Q[3 * i + j];
}

// X = A v for a row-major 3 x 3 matrix
__device__ __forceinline__ void rotate_exact(const float* A, float v0, float v1, float v2, float* X) {
#pragma clang fp contract(off)
  X[0] = fmaf(A[2], v2, fmaf(A[1], v1, A[0] * v0));
  X[1] = fmaf(A[5], v2, fmaf(A[4], v1, A[3] * v0));
  X[2] = fmaf(A[8], v2, fmaf(A[7], v1, A[6] * v0));
}

// pf_pano_crop's ray C = (eta x, eta y, eta - xi) of the image point (x, y), k1 = 1 - xi^2: rho^2, disc, eta.  False where the point has no ray
__device__ __forceinline__ bool usm_ray_exact(float x, float y, float xi, float k1, float* C) {
#pragma clang fp contract(off)
  const float r2 = fmaf(x, x, y * y);
  const float disc = fmaf(k1, r2, 1.f);
  if (!(disc >= 0.f)) return false;
  const float eta = (xi + sqrtf(disc)) / (1.f + r2);
  C[0] = eta * x; C[1] = eta * y; C[2] = eta - xi;
  return true;
}

// pf_pano_rotate's pixel -> direction.  Sine and cosine of the latitude of the point `off` below the top of row `row` of H rows
struct PanoRow { float sl, cl; };
__device__ __forceinline__ PanoRow pano_row(int row, float off, int H) {
#pragma clang fp contract(off)
  PanoRow r;
  sincosf((0.5f - ((float)row + off) / (float)H) * 3.14159265358979323846f, &r.sl, &r.cl);
  return r;
}
// D = (cl so, -sl, cl co) of the point `off` right of the left side of column `col` of W, (so, co) the sine and cosine of its longitude
__device__ __forceinline__ void pano_direction(const PanoRow& r, int col, float off, int W, float* D, float* so, float* co) {
#pragma clang fp contract(off)
  sincosf((((float)col + off) / (float)W - 0.5f) * (2.f * 3.14159265358979323846f), so, co);
  D[0] = r.cl * *so; D[1] = -r.sl; D[2] = r.cl * *co;
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

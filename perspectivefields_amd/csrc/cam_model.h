// Pinhole camera parameters -> perspective fields at one pixel: the per-pixel body of fields_from_params_kernel (elem.hip),
// shared with the pinhole (xi = 0) labels of pano_crop.hip so that both give the same bits for the same fp32 parameters.
// Reference: PanoCam.get_up_general / get_lat_general (utils/panocam.py:451-556).  Quirks kept: up vectors at pixel centres
// (j + 0.5); latitude on linspace(-c, size - c, size) (end points included); elevation == 0 -> constant up field.
// PF_NO_PK_F32 on both helpers: they inline into kernels compiled without the packed-fp32 feature (pf_kernels.h).
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

}  // namespace pf

// The supersampled forms of the three one-source gathers (include/pf_hip.h pf_pano_crop_ss / pf_reproject_ss / pf_pano_rotate_ss, DESIGN.md
// section 25): antialiasing for crops, re-projections and rotations that minify.  VALU and memory bound, no MFMA, no atomics.
// The sample loop, the mean and the stores are gather_ss.h's; the re-projection and the rotation are models plugged into it, the crop keeps its loop
// in its own text and calls gather_ss.h's helpers (DESIGN.md section 31 says why).  A sub-sample is its gather's per-sample model at its point,
// unchanged: ray, validity, source coordinate, tap rule and blend order are those of pano_crop.hip, reproject.hip and pano_rotate.hip, with the
// pixel centre's 1/2 a parameter.  A pixel without a valid sub-sample is 0 (crop, rotation) or `fill` (re-projection).  At S = 1 the offsets are 1/2 exactly and every kernel gives the bits of its parent (tests/test_gpu_gather_samples.py).
// What describes the pixel and not its footprint is taken at the pixel centre with the parent's formulas: the labels of the crop and of the rotation,
// the map of the re-projection.  With an even S the centre is not itself a sub-sample.  The mask of the re-projection is 1 iff a sub-sample is valid.
//   pano_crop_ss_kernel<T, LABELS>, reproject_ss_kernel<T, EXTRAS>, pano_rotate_ss_kernel<T, LABELS>
#include <math.h>
#include <stdint.h>

#include "../../include/pf_hip.h"
#include "cam_model.h"
#include "gather_ss.h"

namespace pf {

namespace {

constexpr float kInv2Pi = 0.15915494309189535f, kInvPi = 0.3183098861837907f, kRad2Deg = 57.29577951308232f;

// ---------------------------------------------------------------- pano_crop.hip's constants
struct CropConsts {
  float R[9];  // camera -> world, row major
  float g[3];  // world up (0, -1, 0) in camera coordinates
  float F, invF, Cx, Cy, xi, yaw_t, sx, sy;
  PinholeFields pin;  // the xi == 0 labels
};

// ---------------------------------------------------------------- reproject.hip's model
struct ReprojConsts {
  float M[9];  // destination camera -> source camera, row major
  float invFd, Cxd, Cyd, xid;
  float Fs, Cxs, Cys, xis, zmin;
};

// M = Rs^T Tm, reproject.hip's `Rs[i] * Tm[j] + Rs[3 + i] * Tm[3 + j] + Rs[6 + i] * Tm[6 + j]` with the rounding steps spelled out.  The sum of
// three products leaves the choice of the one that stays a product to the compiler: in reproject_kernel it is the middle one in the rows i = 0
// and i = 2 and the first one in the row i = 1 (Rs[1] = -sin(roll) makes that sum a difference); inside gather_ss<M> three entries came out
// differently, so reproject_kernel's arrangement is written out here
__device__ __forceinline__ void reproj_matrix(const float* Rs, const float* Tm, float* M) {
#pragma clang fp contract(off)
  for (int j = 0; j < 3; ++j) {
    M[j] = fmaf(Rs[6], Tm[6 + j], fmaf(Rs[0], Tm[j], Rs[3] * Tm[3 + j]));
    M[3 + j] = fmaf(Rs[7], Tm[6 + j], fmaf(Rs[4], Tm[3 + j], Rs[1] * Tm[j]));
    M[6 + j] = fmaf(Rs[8], Tm[6 + j], fmaf(Rs[2], Tm[j], Rs[5] * Tm[3 + j]));
  }
}

template <typename T, bool EXTRAS>
struct ReprojSs {
  using Texel = T;
  using Batch = ReprojSsBatch;
  using Consts = ReprojConsts;

  static __device__ __forceinline__ void setup(const Batch& rb, int o, Consts* c) {
    const int H = rb.d.H, W = rb.d.W, Hs = rb.src.H[o], Ws = rb.src.W[o];
    const float* cs = rb.cam_src + (size_t)o * 7;
    const float* cd = rb.cam_dst + (size_t)o * 7;
    float Rs[9], Rd[9], sy, cy;
    cam_rotation(cs[0], cs[1], Rs);
    cam_rotation(cd[0], cd[1], Rd);
    sincosf(cd[2] - cs[2], &sy, &cy);
    float Tm[9];  // Y(yaw_d - yaw_s) R_d
    for (int j = 0; j < 3; ++j) {
      Tm[j] = cy * Rd[j] + sy * Rd[6 + j];
      Tm[3 + j] = Rd[3 + j];
      Tm[6 + j] = cy * Rd[6 + j] - sy * Rd[j];
    }
    reproj_matrix(Rs, Tm, c->M);
    c->invFd = 1.f / (cd[3] * (float)H);
    c->Cxd = (cd[4] + 0.5f) * (float)W;
    c->Cyd = (cd[5] + 0.5f) * (float)H;
    c->xid = cd[6];
    c->Fs = cs[3] * (float)Hs;
    c->Cxs = (cs[4] + 0.5f) * (float)Ws;
    c->Cys = (cs[5] + 0.5f) * (float)Hs;
    c->xis = cs[6];
    c->zmin = usm_z_min(cs[6]);
  }

  const Batch& rb;
  const Consts& cc;
  const int o;
  const T* __restrict__ src;
  const int Hs, Ws;
  __device__ __forceinline__ ReprojSs(const Batch& b, const Consts& c, int i)
      : rb(b), cc(c), o(i), src(static_cast<const T*>(b.src.p[i])), Hs(b.src.H[i]), Ws(b.src.W[i]) {}

  __device__ __forceinline__ bool ok() const { return true; }  // a non-finite camera fails the positive comparisons below, as in the parent
  __device__ __forceinline__ float empty() const { return rb.fill; }
  __device__ __forceinline__ float row_term(int row, float off) const { return ((float)row + off - cc.Cyd) * cc.invFd; }

  // reproject.hip's steps from the destination point (col + off, .) with normalised row y to the source point (a, b); false where not visible
  __device__ __forceinline__ bool source_point(float y, int col, float off, float* a, float* b) const {
    float X[3], Xs[3], xs, ys;
    if (!usm_ray(((float)col + off - cc.Cxd) * cc.invFd, y, cc.xid, X)) return false;
    to_world(cc.M, X, Xs);
    if (!(Xs[2] > cc.zmin)) return false;
    usm_project(Xs, cc.xis, &xs, &ys);
    *a = cc.Fs * xs + cc.Cxs;
    *b = cc.Fs * ys + cc.Cys;
    return true;
  }

  __device__ __forceinline__ bool sample(float y, int col, float off, float* px) const {
    float a, b;
    if (!source_point(y, col, off, &a, &b)) return false;
    if (!(a >= 0.f && a <= (float)Ws && b >= 0.f && b <= (float)Hs)) return false;  // false for NaN and infinities: no load without a point inside the source
    sample_clamped(src, Hs, Ws, a - 0.5f, b - 0.5f, px);
    return true;
  }

  // the mask, and the map, which is the pixel centre's: reproject.hip's steps at (col + 1/2, row + 1/2)
  __device__ __forceinline__ void finish(int row, int col0, size_t pix, const int* n) const {
    if (!EXTRAS) return;
    const int W = rb.d.W;
    if (rb.valid) store_mask(rb.valid + pix, rb.d.vec, col0, W, n);
    if (!rb.map) return;
    float ma[4], mb[4];
    const float y = row_term(row, 0.5f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ma[k] = mb[k] = __builtin_nanf("");
      if (col0 + k < W) source_point(y, col0 + k, 0.5f, &ma[k], &mb[k]);  // (a, b) are written where the point is visible
    }
    const size_t npx = (size_t)rb.d.H * W;
    float* m = rb.map + pix + (size_t)o * npx;  // [n][2][H][W]
    store_plane4(m, rb.d.vec, col0, W, ma);
    store_plane4(m + npx, rb.d.vec, col0, W, mb);
  }
};

// ---------------------------------------------------------------- pano_rotate.hip's model, the pixel centre's 1/2 a parameter
struct RotConsts {
  float A[9];    // output direction -> source (world) direction, row major
  float g[3];    // world up (0, -1, 0) in the output camera's coordinates: A^T (0, -1, 0)
  float kx, ky;  // W / (2 pi), H / pi: pixels per radian of longitude and of latitude
  int ok;        // 0: a non-finite angle
};

struct RotPixel {
  float ts, tl;      // longitude and latitude of the source point as fractions: lon_s / 2 pi + 1/2 and 1/2 - lat_s / pi
  float ux, uy, lat; // the labels (LABELS only)
};

// the point `off` right of the left side of pixel `col` of an output of W columns, on the row r
template <bool LABELS>
__device__ __forceinline__ RotPixel rot_pixel(const RotConsts& c, const PanoRow& r, int col, float off, int W) {
#pragma clang fp contract(off)
  const float sl = r.sl, cl = r.cl;
  float so, co, D[3], X[3];
  pano_direction(r, col, off, W, D, &so, &co);
  rotate_exact(c.A, D[0], D[1], D[2], X);
  const float nlat = atan2f(X[1], sqrtf(fmaf(X[0], X[0], X[2] * X[2])));  // -lat_s
  RotPixel o;
  o.ts = fmaf(atan2f(X[0], X[2]), kInv2Pi, 0.5f);
  o.tl = fmaf(nlat, kInvPi, 0.5f);
  if (LABELS) {
    o.lat = -nlat * kRad2Deg;
    const float a = fmaf(c.g[0], co, -(c.g[2] * so));
    const float b = -fmaf(c.g[1], cl, sl * fmaf(c.g[0], so, c.g[2] * co));
    const float t2 = fmaf(a, a, b * b);
    const float px = c.kx * a / cl, py = -(c.ky * b);
    const float n = sqrtf(fmaf(px, px, py * py));  // divisions, not a reciprocal: an upright camera gives (0, -1) exactly
    const bool has = t2 >= PF_PANO_UP_MIN_T2;
    o.ux = has ? px / n : __builtin_nanf("");
    o.uy = has ? py / n : __builtin_nanf("");
  }
  return o;
}

template <typename T, bool LABELS>
struct RotSs {
  using Texel = T;
  using Batch = PanoRotSsBatch;
  using Consts = RotConsts;

  static __device__ __forceinline__ void setup(const Batch& rb, int out_i, Consts* c) {
#pragma clang fp contract(off)
    const float* rot = rb.rot + (size_t)out_i * 3;
    pano_rotation(rot, rb.inverse, c->A);
    c->g[0] = -c->A[3]; c->g[1] = -c->A[4]; c->g[2] = -c->A[5];
    c->kx = (float)rb.d.W * kInv2Pi;
    c->ky = (float)rb.d.H * kInvPi;
    c->ok = all_finite(rot, 3) ? 1 : 0;
  }

  const Batch& rb;
  const Consts& rc;
  const int out_i;
  const T* __restrict__ src;
  const int Hs, Ws;
  __device__ __forceinline__ RotSs(const Batch& b, const Consts& c, int i)
      : rb(b), rc(c), out_i(i), src(static_cast<const T*>(b.src.p[i])), Hs(b.src.H[i]), Ws(b.src.W[i]) {}

  __device__ __forceinline__ bool ok() const { return rc.ok != 0; }
  __device__ __forceinline__ float empty() const { return 0.f; }
  __device__ __forceinline__ PanoRow row_term(int row, float off) const { return pano_row(row, off, rb.d.H); }

  __device__ __forceinline__ bool sample(const PanoRow& r, int col, float off, float* px) const {
    const RotPixel o = rot_pixel<false>(rc, r, col, off, rb.d.W);
    pf::sample(src, Hs, Ws, fmaf(o.ts, (float)Ws, -0.5f), fmaf(o.tl, (float)Hs, -0.5f), px);
    return true;
  }

  // the labels are the pixel centre's: pano_rotate.hip's
  __device__ __forceinline__ void finish(int row, int col0, size_t pix, const int*) const {
    if (!LABELS) return;
    const int W = rb.d.W;
    float ux[4], uy[4], lat[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) ux[k] = uy[k] = lat[k] = __builtin_nanf("");
    if (rc.ok) {
      const PanoRow r = row_term(row, 0.5f);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (col0 + k >= W) continue;
        const RotPixel o = rot_pixel<true>(rc, r, col0 + k, 0.5f, W);
        ux[k] = o.ux; uy[k] = o.uy; lat[k] = o.lat;
      }
    }
    store_labels(rb.up, rb.lat, rb.d.vec, out_i, (size_t)rb.d.H * W, pix, col0, W, ux, uy, lat);
  }
};

}  // namespace

// The crop keeps gather_ss<M>'s loop in its own text: as a model the compiler fused the other product of bilerp_rgb's `(1 - fu) t00 + fu t01`
// (other bits than pano_crop_kernel's), and with that blend spelled out the kernel was 15 - 20 % slower on the timed crop workload (DESIGN.md
// section 31).  A change to gather_ss<M>'s loop or rules has to be made here as well
template <typename T, bool LABELS>
__global__ __launch_bounds__(256) void pano_crop_ss_kernel(PanoSsBatch pb) {
  __shared__ CropConsts cc;
  const int crop = blockIdx.y;
  const int H = pb.d.H, W = pb.d.W;
  if (threadIdx.x == 0) {
    const float* cam = pb.cam + (size_t)crop * 7;
    const float roll = cam[0], pitch = cam[1], yaw = cam[2], f = cam[3], rcx = cam[4], rcy = cam[5], xi = cam[6];
    float sr, cr, sp, cp, R[9];
    sincosf(roll, &sr, &cr);
    sincosf(pitch, &sp, &cp);
    cam_rotation(sr, cr, sp, cp, R);
    for (int k = 0; k < 9; ++k) cc.R[k] = R[k];
    cc.g[0] = -R[3]; cc.g[1] = -R[4]; cc.g[2] = -R[5];
    cc.F = f * (float)H;
    cc.invF = 1.f / cc.F;
    cc.Cx = (rcx + 0.5f) * (float)W;
    cc.Cy = (rcy + 0.5f) * (float)H;
    cc.xi = xi;
    cc.yaw_t = yaw * kInv2Pi + 0.5f;
    cc.sx = W > 1 ? (float)W / (float)(W - 1) : 0.f;
    cc.sy = H > 1 ? (float)H / (float)(H - 1) : 0.f;
    if (LABELS) cc.pin = pinhole_fields_setup(roll, pitch, f, rcx, rcy, H, W);
  }
  __syncthreads();
  const int tpr = pb.d.tpr;  // threads per tile row; the tile is (4 tpr) x (256 / tpr) pixels
  const int tile_x = blockIdx.x % pb.d.tiles_x, tile_y = blockIdx.x / pb.d.tiles_x;
  const int row = tile_y * (256 / tpr) + threadIdx.x / tpr;
  const int col0 = tile_x * 4 * tpr + (threadIdx.x % tpr) * 4;
  if (row >= H || col0 >= W) return;
  const T* __restrict__ pano = static_cast<const T*>(pb.src.p[crop]);
  const int Hp = pb.src.H[crop], Wp = pb.src.W[crop];
  const float xi = cc.xi;
  const int S = pb.samples;
  const float fS = (float)S;

  float acc[4][3];
  int n[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc[k][0] = acc[k][1] = acc[k][2] = -0.f;
    n[k] = 0;
  }
  for (int i = 0; i < S; ++i) {
    const float y = ((float)row + sub_offset(i, fS) - cc.Cy) * cc.invF;
    for (int j = 0; j < S; ++j) {
      const float oj = sub_offset(j, fS);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int col = col0 + k;
        if (col >= W) continue;
        float X[3];
        if (usm_ray(((float)col + oj - cc.Cx) * cc.invF, y, xi, X)) {
          float Xw[3], px[3];
          to_world(cc.R, X, Xw);
          float t = cc.yaw_t + atan2f(Xw[0], Xw[2]) * kInv2Pi;
          t -= floorf(t);
          const float u = t * (float)Wp - 0.5f;
          const float v = (0.5f + atan2f(Xw[1], sqrtf(Xw[0] * Xw[0] + Xw[2] * Xw[2])) * kInvPi) * (float)Hp - 0.5f;
          sample(pano, Hp, Wp, u, v, px);
          acc[k][0] += px[0]; acc[k][1] += px[1]; acc[k][2] += px[2];
          ++n[k];
        }
      }
    }
  }

  float img[4][3], ux[4], uy[4], lat[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int col = col0 + k;
    mean_of(acc[k], n[k], 0.f, img[k]);
    ux[k] = uy[k] = lat[k] = __builtin_nanf("");
    if (!LABELS || col >= W) continue;
    float X[3];  // the labels are the pixel's: pano_crop.hip's at (col + 1/2, row + 1/2) and at the linspace point
    if (xi == 0.f) {
      const FieldsPixel o = pinhole_fields_at(cc.pin, row, col);
      ux[k] = o.ux;
      uy[k] = o.uy;
      lat[k] = o.lat;
    } else {
      if (usm_ray(((float)col + 0.5f - cc.Cx) * cc.invF, ((float)row + 0.5f - cc.Cy) * cc.invF, xi, X)) usm_up_of_ray(X, cc.g, xi, &ux[k], &uy[k]);
      if (usm_ray(((float)col * cc.sx - cc.Cx) / cc.F, ((float)row * cc.sy - cc.Cy) / cc.F, xi, X)) lat[k] = usm_lat_of_ray(X, cc.R);
    }
  }

  const size_t npx = (size_t)H * W, pix = (size_t)crop * npx + (size_t)row * W + col0;
  store_image(static_cast<T*>(pb.img) + pix * 3, pb.d.vec, col0, W, img);
  if (LABELS) store_labels(pb.up, pb.lat, pb.d.vec, crop, npx, pix, col0, W, ux, uy, lat);
}

template <typename T, bool EXTRAS>
__global__ __launch_bounds__(256) void reproject_ss_kernel(ReprojSsBatch rb) { gather_ss<ReprojSs<T, EXTRAS>>(rb); }

template <typename T, bool LABELS>
__global__ __launch_bounds__(256) void pano_rotate_ss_kernel(PanoRotSsBatch rb) { gather_ss<RotSs<T, LABELS>>(rb); }

void launch_pano_crop_ss(const PanoSsBatch& pb, int dtype, hipStream_t s) {
  if (pb.up) launch_ss(pano_crop_ss_kernel<uint8_t, true>, pano_crop_ss_kernel<float, true>, pb, dtype, s);
  else launch_ss(pano_crop_ss_kernel<uint8_t, false>, pano_crop_ss_kernel<float, false>, pb, dtype, s);
}

void launch_reproject_ss(const ReprojSsBatch& rb, int dtype, hipStream_t s) {
  if (rb.valid || rb.map) launch_ss(reproject_ss_kernel<uint8_t, true>, reproject_ss_kernel<float, true>, rb, dtype, s);
  else launch_ss(reproject_ss_kernel<uint8_t, false>, reproject_ss_kernel<float, false>, rb, dtype, s);
}

void launch_pano_rotate_ss(const PanoRotSsBatch& rb, int dtype, hipStream_t s) {
  if (rb.up) launch_ss(pano_rotate_ss_kernel<uint8_t, true>, pano_rotate_ss_kernel<float, true>, rb, dtype, s);
  else launch_ss(pano_rotate_ss_kernel<uint8_t, false>, pano_rotate_ss_kernel<float, false>, rb, dtype, s);
}

}  // namespace pf

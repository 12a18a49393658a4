// Fisheye and dual-fisheye frames as a target: equirectangular panoramas -> the frames of one or two lenses, and the perspective fields of a fisheye
// camera (include/pf_hip.h pf_pano_to_fisheye / pf_fisheye_fields).  VALU and memory bound, no MFMA, no atomics, no workspace.
//   pano_to_fisheye_kernel<T, LABELS>  a model of gather_ss.h, which owns the launch shape, the `samples` loop, the mean (`fill` without a valid
//                                      sub-sample) and the image's stores.  Lane 0 computes per lens Q, R, g, the intrinsics and r_max into LDS.  A
//                                      sub-sample goes pixel -> lens direction X (fisheye_unproject) -> world direction D = Q X -> panorama tap
//                                      (gather.h `sample`).  finish() stores the mask and, with LABELS, the labels of the pixel centre.
//   fisheye_fields_kernel              the labels alone, no source: the same two per-pixel functions, so the same bits as the LABELS path.
// The projection kind is a block-uniform run-time switch; the Newton iteration of the Kannala-Brandt polynomial has a fixed count
// (PF_FISHEYE_NEWTON_STEPS) and is skipped per lens where k1 = ... = k4 = 0.
// Model (the contract; tests/test_fisheye_target_ref.py states it in fp64), at the image point (a, b), per lens l = 0, 1 in that order:
//   dx = a - Cx, dy = b - Cy, r = sqrt(fma(dx, dx, dy dy)); the lens owns the point iff it is on and r_max - r > 0, the first owner wins
//   rho = r / F, td = rho | 2 asin(min(rho / 2, 1)) | 2 atan(rho / 2); t = td without a polynomial, else the clamped Newton steps from min(td, t_max)
//   (cp, sp) = (dx, dy) / r, (1, 0) where r = 0; X = (sin t cp, sin t sp, cos t)
//   image    D = Q X, u = (atan2(D.x, D.z) / 2 pi + 1/2) Wp - 1/2, v = (atan2(D.y, hypot(D.x, D.z)) / pi + 1/2) Hp - 1/2, `sample` at (u, v)
//   labels   W = R X, latitude = -atan2(W.y, hypot(W.x, W.z)) in degrees; ge = g . e_theta, gp = g . e_phi with e_theta = (cos t cp, cos t sp, -sin t),
//            e_phi = (-sp, cp, 0) (so t_g = g - (g . X) X = ge e_theta + gp e_phi and |t_g|^2 = ge^2 + gp^2); m' = rho'(td) P'(t), mt = rho / sin t
//            (m' where r = 0); up ~ m' ge (cp, sp) + mt gp (-sp, cp) normalised, NaN where ge^2 + gp^2 < PF_PANO_UP_MIN_T2
// Every rounding step of the setup and of the two per-pixel functions is spelled out (contraction off, fmaf where a fused step is meant).
#include <math.h>
#include <stdint.h>

#include "../../include/pf_hip.h"
#include "cam_model.h"
#include "fisheye_model.h"
#include "gather_ss.h"

// every rounding step of this unit's setup and per-pixel functions is spelled out: no contraction in what follows, fmaf where a fused step is meant
#pragma clang fp contract(off)

namespace pf {

namespace {

constexpr float kInv2Pi = 0.15915494309189535f, kInvPi = 0.3183098861837907f, kRad2Deg = 57.29577951308232f;

struct TargetLens {
  float Q[9];  // lens -> world, Y(yaw) R_pitch R_roll, row major: the image
  float R[9];  // R_pitch R_roll: the labels, which the yaw does not enter
  float g[3];  // world up (0, -1, 0) in the lens' coordinates: R^T (0, -1, 0)
  float F, Cx, Cy, tmax, k1, k2, k3, k4;
  float rmax;  // F rho(P(theta_max)): the radius of the image circle
  int on;      // 0: a non-finite entry or theta_max <= 0: the lens owns nothing
  int poly;    // 0: k1 = ... = k4 = 0, theta = theta_d
};

struct TargetConsts {
  TargetLens lens[PF_FISHEYE_MAX_LENSES];
  int any;  // 0: no lens is on
};

__device__ __forceinline__ void target_lens_setup(const float* __restrict__ lens, int kind, TargetLens* c) {
  world_rotation(lens[0], lens[1], lens[2], c->Q);
  cam_rotation(lens[0], lens[1], c->R);
  c->g[0] = -c->R[3]; c->g[1] = -c->R[4]; c->g[2] = -c->R[5];
  c->F = lens[3]; c->Cx = lens[4]; c->Cy = lens[5]; c->tmax = lens[6];
  c->k1 = lens[7]; c->k2 = lens[8]; c->k3 = lens[9]; c->k4 = lens[10];
  c->rmax = c->F * fisheye_rho(kind, fisheye_poly(c->tmax, c->k1, c->k2, c->k3, c->k4));
  c->on = fisheye_lens_on(lens) ? 1 : 0;
  c->poly = (c->k1 != 0.f || c->k2 != 0.f || c->k3 != 0.f || c->k4 != 0.f) ? 1 : 0;
}

__device__ __forceinline__ void target_setup(const float* __restrict__ lens, int kind, TargetConsts* c) {
  for (int l = 0; l < PF_FISHEYE_MAX_LENSES; ++l) target_lens_setup(lens + l * PF_FISHEYE_LENS_FLOATS, kind, &c->lens[l]);
  c->any = (c->lens[0].on | c->lens[1].on) ? 1 : 0;
}

// dy of a point per lens: what depends on the point's row alone
struct LensRow { float dy[PF_FISHEYE_MAX_LENSES]; };
__device__ __forceinline__ LensRow lens_row(const TargetLens* lens, int row, float off) {
  LensRow r;
  const float b = (float)row + off;
#pragma unroll
  for (int l = 0; l < PF_FISHEYE_MAX_LENSES; ++l) r.dy[l] = b - lens[l].Cy;
  return r;
}

// an image point in the lens that owns it
struct FisheyePoint {
  float X[3];           // its direction in the lens' coordinates
  float cp, sp, st, ct; // cosine and sine of its azimuth about the lens axis and of theta
  float t, td, rho;     // theta, theta_d, r / F
  int lens;             // the owner
  bool centre;          // r = 0
};

// the inverse projection of the point `a` right of the frame's left side on the row r: false where no lens owns it
__device__ __forceinline__ bool fisheye_unproject(const TargetLens* lens, int kind, float a, const LensRow& r, FisheyePoint* p) {
#pragma unroll
  for (int l = 0; l < PF_FISHEYE_MAX_LENSES; ++l) {
    const TargetLens& c = lens[l];
    if (!c.on) continue;
    const float dx = a - c.Cx, dy = r.dy[l];
    const float rad = sqrtf(fmaf(dx, dx, dy * dy));
    if (!(c.rmax - rad > 0.f)) continue;  // a positive comparison: a NaN owns nothing
    const float rho = rad / c.F;
    const float td = fisheye_rho_inverse(kind, rho);
    float t = td;
    if (c.poly) {
      t = fminf(td, c.tmax);
      for (int s = 0; s < PF_FISHEYE_NEWTON_STEPS; ++s) {
        const float f = fisheye_poly(t, c.k1, c.k2, c.k3, c.k4) - td;
        t = fminf(fmaxf(t - f / fisheye_poly_slope(t, c.k1, c.k2, c.k3, c.k4), 0.f), c.tmax);
      }
    }
    p->centre = !(rad > 0.f);
    p->cp = p->centre ? 1.f : dx / rad;
    p->sp = p->centre ? 0.f : dy / rad;
    sincosf(t, &p->st, &p->ct);
    p->X[0] = p->st * p->cp; p->X[1] = p->st * p->sp; p->X[2] = p->ct;
    p->t = t; p->td = td; p->rho = rho;
    p->lens = l;
    return true;
  }
  return false;
}

// the perspective fields at a point of the lens c that owns it: the up vector in the image and the latitude in degrees
__device__ __forceinline__ void fisheye_labels(const TargetLens& c, int kind, const FisheyePoint& p, float* ux, float* uy, float* lat) {
  float Xw[3];
  rotate_exact(c.R, p.X[0], p.X[1], p.X[2], Xw);
  *lat = -atan2f(Xw[1], sqrtf(fmaf(Xw[0], Xw[0], Xw[2] * Xw[2]))) * kRad2Deg;
  const float ge = fmaf(c.g[2], -p.st, fmaf(c.g[1], p.ct * p.sp, c.g[0] * (p.ct * p.cp)));
  const float gp = fmaf(c.g[1], p.cp, -(c.g[0] * p.sp));
  const float t2 = fmaf(ge, ge, gp * gp);
  const float ms = fisheye_rho_slope(kind, p.td) * (c.poly ? fisheye_poly_slope(p.t, c.k1, c.k2, c.k3, c.k4) : 1.f);
  const float mt = p.centre ? ms : p.rho / p.st;
  const float A = ms * ge, B = mt * gp;
  const float px = fmaf(A, p.cp, -(B * p.sp)), py = fmaf(A, p.sp, B * p.cp);
  const float n = sqrtf(fmaf(px, px, py * py));
  const bool has = t2 >= PF_PANO_UP_MIN_T2;
  *ux = has ? px / n : __builtin_nanf("");
  *uy = has ? py / n : __builtin_nanf("");
}

// the labels of the 4 pixels (row, col0 ...) of output out_i at their centres; NaN in all three planes without an owner
__device__ __forceinline__ void labels4(const TargetConsts& tc, int kind, float* up, float* lat, int vec, int out_i, int H, int W, int row, int col0,
                                        size_t pix) {
  float ux[4], uy[4], la[4];
  const LensRow r = lens_row(tc.lens, row, 0.5f);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    ux[k] = uy[k] = la[k] = __builtin_nanf("");
    if (col0 + k >= W || !tc.any) continue;
    FisheyePoint p;
    if (!fisheye_unproject(tc.lens, kind, (float)(col0 + k) + 0.5f, r, &p)) continue;
    fisheye_labels(tc.lens[p.lens], kind, p, &ux[k], &uy[k], &la[k]);
  }
  store_labels(up, lat, vec, out_i, (size_t)H * W, pix, col0, W, ux, uy, la);
}

template <typename T, bool LABELS>
struct PanoToFisheye {
  using Texel = T;
  using Batch = PanoToFisheyeBatch;
  using Consts = TargetConsts;

  static __device__ __forceinline__ void setup(const Batch& fb, int out_i, Consts* c) {
    target_setup(fb.lens + (size_t)out_i * PF_FISHEYE_MAX_LENSES * PF_FISHEYE_LENS_FLOATS, fb.kind, c);
  }

  const Batch& fb;
  const Consts& tc;
  const int out_i;
  const T* __restrict__ src;
  const int Hp, Wp, kind;
  __device__ __forceinline__ PanoToFisheye(const Batch& b, const Consts& c, int i)
      : fb(b), tc(c), out_i(i), src(static_cast<const T*>(b.src.p[i])), Hp(b.src.H[i]), Wp(b.src.W[i]), kind(b.kind) {}

  __device__ __forceinline__ bool ok() const { return tc.any != 0; }
  __device__ __forceinline__ float empty() const { return fb.fill; }
  __device__ __forceinline__ LensRow row_term(int row, float off) const { return lens_row(tc.lens, row, off); }

  __device__ __forceinline__ bool sample(const LensRow& r, int col, float off, float* px) const {
    FisheyePoint p;
    if (!fisheye_unproject(tc.lens, kind, (float)col + off, r, &p)) return false;
    float D[3];
    rotate_exact(tc.lens[p.lens].Q, p.X[0], p.X[1], p.X[2], D);
    const float ts = fmaf(atan2f(D[0], D[2]), kInv2Pi, 0.5f);
    const float tl = fmaf(atan2f(D[1], sqrtf(fmaf(D[0], D[0], D[2] * D[2]))), kInvPi, 0.5f);
    pf::sample(src, Hp, Wp, fmaf(ts, (float)Wp, -0.5f), fmaf(tl, (float)Hp, -0.5f), px);
    return true;
  }

  __device__ __forceinline__ void finish(int row, int col0, size_t pix, const int* n) const {
    if (fb.valid) store_mask(fb.valid + pix, fb.d.vec, col0, fb.d.W, n);
    if (LABELS) labels4(tc, kind, fb.up, fb.lat, fb.d.vec, out_i, fb.d.H, fb.d.W, row, col0, pix);
  }
};

}  // namespace

template <typename T, bool LABELS>
__global__ __launch_bounds__(256) void pano_to_fisheye_kernel(PanoToFisheyeBatch fb) { gather_ss<PanoToFisheye<T, LABELS>>(fb); }

__global__ __launch_bounds__(256) void fisheye_fields_kernel(FisheyeFieldsBatch fb) {
  __shared__ TargetConsts tc;
  const int out_i = blockIdx.y;
  const int H = fb.d.H, W = fb.d.W;
  if (threadIdx.x == 0) target_setup(fb.lens + (size_t)out_i * PF_FISHEYE_MAX_LENSES * PF_FISHEYE_LENS_FLOATS, fb.kind, &tc);
  __syncthreads();
  const int tpr = fb.d.tpr;  // threads per tile row; the tile is (4 tpr) x (256 / tpr) pixels
  const int tile_x = blockIdx.x % fb.d.tiles_x, tile_y = blockIdx.x / fb.d.tiles_x;
  const int row = tile_y * (256 / tpr) + threadIdx.x / tpr;
  const int col0 = tile_x * 4 * tpr + (threadIdx.x % tpr) * 4;
  if (row >= H || col0 >= W) return;
  const size_t pix = (size_t)out_i * ((size_t)H * W) + (size_t)row * W + col0;
  labels4(tc, fb.kind, fb.up, fb.lat, fb.d.vec, out_i, H, W, row, col0, pix);
}

void launch_pano_to_fisheye(const PanoToFisheyeBatch& fb, int dtype, hipStream_t s) {
  if (fb.up) launch_ss(pano_to_fisheye_kernel<uint8_t, true>, pano_to_fisheye_kernel<float, true>, fb, dtype, s);
  else launch_ss(pano_to_fisheye_kernel<uint8_t, false>, pano_to_fisheye_kernel<float, false>, fb, dtype, s);
}

void launch_fisheye_fields(const FisheyeFieldsBatch& fb, hipStream_t s) {
  const dim3 grid((unsigned)(fb.d.tiles_x * fb.d.tiles_y), (unsigned)fb.d.n), block(256);
  hipLaunchKernelGGL(fisheye_fields_kernel, grid, block, 0, s, fb);
}

}  // namespace pf

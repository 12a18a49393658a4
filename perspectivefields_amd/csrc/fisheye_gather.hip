// Fisheye and dual-fisheye frames as a source: camera views and equirectangular panoramas out of one or two lenses of a frame (include/pf_hip.h
// pf_fisheye_crop / pf_fisheye_to_pano): two more image gathers of gather.h.  VALU and memory bound, no MFMA, no atomics, no
// workspace.
//   fisheye_crop_kernel<T>     views of cameras (roll, pitch, yaw, rel_focal, rel_cx, rel_cy, xi): pf_pano_crop's ray C, world direction D = Qc C with
//                              Qc = Y(yaw) R_pitch R_roll, the frame's value in D
//   fisheye_to_pano_kernel<T>  panoramas: pf_pano_rotate's pixel -> direction D0 and D = A D0, the frame's value in D
//       both are models of gather_ss.h, which owns the launch shape, the `samples` loop, the mean (`fill` without a valid sub-sample) and the stores;
//       the ray, the rotations and the pixel -> direction are cam_model.h's.  Lane 0 computes per lens M = Ql^T Qc or Ql^T A, so that a sample goes
//       from the camera ray or the panorama direction into the lens in one 3 x 3 product, and the lens' intrinsics.  The projection kind is a
//       block-uniform run-time switch.
// The value of a frame in a direction (the contract; tests/test_fisheye_ref.py states it in fp64), per lens l = 0, 1 in that order:
//   angle    X = M v, h = sqrt(fma(X0, X0, X1 X1)), t = atan2f(h, X2)
//   point    td = t * fma(t2, fma(t2, fma(t2, fma(t2, k4, k3), k2), k1), 1) with t2 = t t;  r = F rho(td), rho = td | 2 sinf(td / 2) | 2 tanf(td / 2);
//            s = r / h;  (a, b) = (fma(s, X0, Cx), fma(s, X1, Cy)), (Cx, Cy) where h == 0
//   covered  the lens is on (its 12 entries finite, theta_max > 0) and theta_max - t > 0 and 0 <= a <= Ws and 0 <= b <= Hs: positive comparisons
//            only, so that a NaN covers nothing and no load is issued without a point inside the frame
//   weight   w = fminf((theta_max - t) / band, 1) for band > 0, else 1
//   colour   c = sample_clamped at (a - 1/2, b - 1/2)
//   S = S + w, C = fma(w, c, C) from 0; valid iff S > 0, value C / S.
// Every rounding step of the setup and of the per-sample function is spelled out (contraction off, fmaf where a fused step is meant).
#include <math.h>
#include <stdint.h>

#include "../../include/pf_hip.h"
#include "cam_model.h"
#include "gather_ss.h"

// every rounding step of this unit's setup and per-sample functions is spelled out: no contraction in what follows, fmaf where a fused step is meant
#pragma clang fp contract(off)

namespace pf {

namespace {

struct LensConsts {
  float M[9];  // camera ray or panorama direction -> lens coordinates, row major
  float F, Cx, Cy, tmax, k1, k2, k3, k4, band;
  int on;      // 0: a non-finite entry or theta_max <= 0: the lens covers nothing
};

struct FisheyeConsts {
  LensConsts lens[PF_FISHEYE_MAX_LENSES];
  float invF, Cx, Cy, xi;  // the view's camera (fisheye_crop_kernel)
  int ok;                  // 0: a non-finite camera or angle entry
};

// the constants of lens l of output out_i: M = Ql^T A for the 3 x 3 matrix A (row major) that takes the sample's vector into the world
__device__ __forceinline__ void lens_setup(const float* __restrict__ lens, const float* A, LensConsts* c) {
  float Q[9];
  world_rotation(lens[0], lens[1], lens[2], Q);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) c->M[3 * i + j] = fmaf(Q[6 + i], A[6 + j], fmaf(Q[3 + i], A[3 + j], Q[i] * A[j]));
  c->F = lens[3]; c->Cx = lens[4]; c->Cy = lens[5]; c->tmax = lens[6];
  c->k1 = lens[7]; c->k2 = lens[8]; c->k3 = lens[9]; c->k4 = lens[10];
  c->band = lens[11];
  c->on = (all_finite(lens, PF_FISHEYE_LENS_FLOATS) && lens[6] > 0.f) ? 1 : 0;
}

// the frame's value in the direction whose vector is v (a camera ray or a panorama direction): false where no lens covers it
template <typename T>
__device__ __forceinline__ bool fisheye_sample(const T* __restrict__ src, int Hs, int Ws, int kind, const LensConsts* lens, float v0, float v1, float v2,
                                               float* out) {
  const float wmax = (float)Ws, hmax = (float)Hs;
  float S = 0.f, C[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int l = 0; l < PF_FISHEYE_MAX_LENSES; ++l) {
    const LensConsts& c = lens[l];
    if (!c.on) continue;
    float X[3];
    rotate_exact(c.M, v0, v1, v2, X);
    const float h = sqrtf(fmaf(X[0], X[0], X[1] * X[1]));
    const float t = atan2f(h, X[2]);
    const float margin = c.tmax - t;
    if (!(margin > 0.f)) continue;
    const float t2 = t * t;
    const float td = t * fmaf(t2, fmaf(t2, fmaf(t2, fmaf(t2, c.k4, c.k3), c.k2), c.k1), 1.f);
    const float rho = kind == PF_FISHEYE_EQUIDISTANT ? td : kind == PF_FISHEYE_EQUISOLID ? 2.f * sinf(td * 0.5f) : 2.f * tanf(td * 0.5f);
    const float s = c.F * rho / h;
    const float a = h > 0.f ? fmaf(s, X[0], c.Cx) : c.Cx, b = h > 0.f ? fmaf(s, X[1], c.Cy) : c.Cy;
    if (!(a >= 0.f && a <= wmax && b >= 0.f && b <= hmax)) continue;  // false for NaN and infinities: no load without a point inside the frame
    const float w = c.band > 0.f ? fminf(margin / c.band, 1.f) : 1.f;
    float px[3];
    sample_clamped(src, Hs, Ws, a - 0.5f, b - 0.5f, px);
    S = S + w;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) C[ch] = fmaf(w, px[ch], C[ch]);
  }
  if (!(S > 0.f)) return false;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) out[ch] = C[ch] / S;
  return true;
}

// ---------------------------------------------------------------- the two models of gather_ss.h: an empty pixel is `fill`, the mask is stored beside the image
template <typename T, class BatchT>
struct FisheyeSource {  // what both keep per thread
  using Texel = T;
  using Batch = BatchT;
  using Consts = FisheyeConsts;

  static __device__ __forceinline__ const float* lens_of(const Batch& fb, int out_i, int l) {
    return fb.lens + ((size_t)out_i * PF_FISHEYE_MAX_LENSES + l) * PF_FISHEYE_LENS_FLOATS;
  }

  const Batch& fb;
  const Consts& fc;
  const T* __restrict__ src;
  const int Hs, Ws, kind;
  __device__ __forceinline__ FisheyeSource(const Batch& b, const Consts& c, int i)
      : fb(b), fc(c), src(static_cast<const T*>(b.src.p[i])), Hs(b.src.H[i]), Ws(b.src.W[i]), kind(b.kind) {}

  __device__ __forceinline__ bool ok() const { return fc.ok != 0; }
  __device__ __forceinline__ float empty() const { return fb.fill; }
  __device__ __forceinline__ void finish(int, int col0, size_t pix, const int* n) const {
    if (fb.valid) store_mask(fb.valid + pix, fb.d.vec, col0, fb.d.W, n);
  }
};

// views of cameras: pf_pano_crop's ray (usm_ray_exact) C, M = Ql^T Qc takes it into the lens
template <typename T>
struct FisheyeCrop : FisheyeSource<T, FisheyeCropBatch> {
  using Base = FisheyeSource<T, FisheyeCropBatch>;

  static __device__ __forceinline__ void setup(const FisheyeCropBatch& fb, int out_i, FisheyeConsts* c) {
    const float* cam = fb.cam + (size_t)out_i * 7;
    float Q[9];
    world_rotation(cam[0], cam[1], cam[2], Q);
    for (int l = 0; l < PF_FISHEYE_MAX_LENSES; ++l) lens_setup(Base::lens_of(fb, out_i, l), Q, &c->lens[l]);
    c->invF = 1.f / (cam[3] * (float)fb.d.H);
    c->Cx = (cam[4] + 0.5f) * (float)fb.d.W;
    c->Cy = (cam[5] + 0.5f) * (float)fb.d.H;
    c->xi = cam[6];
    c->ok = all_finite(cam, 7) ? 1 : 0;
  }

  const float xi, k1;
  __device__ __forceinline__ FisheyeCrop(const FisheyeCropBatch& b, const FisheyeConsts& c, int i) : Base(b, c, i), xi(c.xi), k1(1.f - c.xi * c.xi) {}

  __device__ __forceinline__ float row_term(int row, float off) const { return ((float)row + off - this->fc.Cy) * this->fc.invF; }
  __device__ __forceinline__ bool sample(float y, int col, float off, float* px) const {
    float C[3];
    if (!usm_ray_exact(((float)col + off - this->fc.Cx) * this->fc.invF, y, xi, k1, C)) return false;
    return fisheye_sample(this->src, this->Hs, this->Ws, this->kind, this->fc.lens, C[0], C[1], C[2], px);
  }
};

// panoramas: pf_pano_rotate's pixel -> direction (pano_row, pano_direction) D, M = Ql^T A takes it into the lens
template <typename T>
struct FisheyePano : FisheyeSource<T, FisheyePanoBatch> {
  using Base = FisheyeSource<T, FisheyePanoBatch>;

  static __device__ __forceinline__ void setup(const FisheyePanoBatch& fb, int out_i, FisheyeConsts* c) {
    const float* rot = fb.rot + (size_t)out_i * 3;
    float A[9];
    pano_rotation(rot, fb.inverse, A);
    for (int l = 0; l < PF_FISHEYE_MAX_LENSES; ++l) lens_setup(Base::lens_of(fb, out_i, l), A, &c->lens[l]);
    c->ok = all_finite(rot, 3) ? 1 : 0;
  }

  using Base::Base;

  __device__ __forceinline__ PanoRow row_term(int row, float off) const { return pano_row(row, off, this->fb.d.H); }
  __device__ __forceinline__ bool sample(const PanoRow& r, int col, float off, float* px) const {
    float so, co, D[3];
    pano_direction(r, col, off, this->fb.d.W, D, &so, &co);
    return fisheye_sample(this->src, this->Hs, this->Ws, this->kind, this->fc.lens, D[0], D[1], D[2], px);
  }
};

}  // namespace

template <typename T>
__global__ __launch_bounds__(256) void fisheye_crop_kernel(FisheyeCropBatch fb) { gather_ss<FisheyeCrop<T>>(fb); }

template <typename T>
__global__ __launch_bounds__(256) void fisheye_to_pano_kernel(FisheyePanoBatch fb) { gather_ss<FisheyePano<T>>(fb); }

void launch_fisheye_crop(const FisheyeCropBatch& fb, int dtype, hipStream_t s) {
  launch_ss(fisheye_crop_kernel<uint8_t>, fisheye_crop_kernel<float>, fb, dtype, s);
}

void launch_fisheye_to_pano(const FisheyePanoBatch& fb, int dtype, hipStream_t s) {
  launch_ss(fisheye_to_pano_kernel<uint8_t>, fisheye_to_pano_kernel<float>, fb, dtype, s);
}

}  // namespace pf
